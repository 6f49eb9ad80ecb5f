// What next_plaid.hpp's MmapIndex::append hands np_hip_index_append: exactly the doc lengths, codes and residuals that the
// update_append before it wrote to the directory -- read back from the chunk files, not encoded a second time -- and what
// append_arrays / reserve / capacity pass through.  With the host compiler alone: the np_hip_* entries are recording stubs in
// this translation unit (no library is linked), and the stub of np_hip_index_update_append changes the directory the way
// update_index does (update.rs:771-1120): the new documents join the last chunk and fill a chunk of their own behind it.
// Built with -fsanitize=address,undefined.  argv[1] = an empty directory to work in.
#include <cstdio>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

int failed = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

struct stub {
  int dummy;
} the_index;
const int PD = 4;   // dim 8, nbits 4
std::string dir;
std::vector<std::string> calls;
int64_t n_docs = 0, n_tokens = 0;   // what the stub handle and the directory hold
// what the stubbed update "encodes" for the call's documents, and what np_hip_index_append received
std::vector<int64_t> enc_lens, enc_codes, got_lens, got_codes;
std::vector<uint8_t> enc_res, got_res;
int64_t got_reserve[2] = {-1, -1};
bool forget_a_chunk = false, refuse_handle = false;

void write_file(const std::string& path, const std::string& bytes) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) {
    std::printf("cannot write %s\n", path.c_str());
    std::exit(2);
  }
  std::fclose(f);
}
std::string npy(const char* descr, const std::string& shape, const void* data, size_t bytes, int version) {
  std::string h = std::string("{'descr': '") + descr + "', 'fortran_order': False, 'shape': (" + shape + "), }";
  const size_t pre = version == 1 ? 10 : 12;
  while ((pre + h.size() + 1) % 64) h += ' ';
  h += '\n';
  std::string out("\x93NUMPY", 6);
  out += (char)version;
  out += (char)0;
  for (size_t i = 0; i < (version == 1 ? 2u : 4u); ++i) out += (char)((h.size() >> (8 * i)) & 0xFF);
  return out + h + std::string((const char*)data, bytes);
}
void write_chunk(int64_t c, const std::vector<int64_t>& lens, const std::vector<int64_t>& codes, const std::vector<uint8_t>& res,
                 int version) {
  std::string j = "[";
  for (size_t i = 0; i < lens.size(); ++i) j += (i ? "," : "") + std::to_string((long long)lens[i]);
  const std::string stem = dir + "/" + std::to_string((long long)c);
  write_file(dir + "/doclens." + std::to_string((long long)c) + ".json", j + "]");
  write_file(stem + ".codes.npy", npy("<i8", std::to_string(codes.size()) + ",", codes.data(), codes.size() * 8, version));
  write_file(stem + ".residuals.npy",
             npy("|u1", std::to_string(codes.size()) + ", " + std::to_string(PD), res.data(), res.size(), version));
}
void write_meta(int64_t chunks) {
  write_file(dir + "/metadata.json", "{\n  \"num_chunks\": " + std::to_string((long long)chunks) + ",\n  \"nbits\": 4,\n  \"num_partitions\": 16,\n"
             "  \"num_embeddings\": " + std::to_string((long long)n_tokens) + ",\n  \"avg_doclen\": 2.5,\n  \"num_documents\": " +
             std::to_string((long long)n_docs) + ",\n  \"embedding_dim\": 8\n}");
}
void tokens_of(const std::vector<int64_t>& lens, int64_t salt, std::vector<int64_t>* codes, std::vector<uint8_t>* res) {
  int64_t t = 0;
  for (int64_t l : lens) t += l;
  codes->resize((size_t)t);
  res->resize((size_t)t * PD);
  for (int64_t i = 0; i < t; ++i) (*codes)[(size_t)i] = (salt * 7 + i * 5) % 16;
  for (size_t i = 0; i < res->size(); ++i) (*res)[i] = (uint8_t)(salt * 31 + (int64_t)i * 13);
}

// the base directory: chunk 0 (full) and chunk 1 (short: an update appends to it)
std::vector<int64_t> c1_lens{3, 0, 2}, c1_codes;
std::vector<uint8_t> c1_res;
void write_base() {
  std::vector<int64_t> l0{2, 4, 1}, k0;
  std::vector<uint8_t> r0;
  tokens_of(l0, 1, &k0, &r0);
  tokens_of(c1_lens, 2, &c1_codes, &c1_res);
  write_chunk(0, l0, k0, r0, 1);
  write_chunk(1, c1_lens, c1_codes, c1_res, 1);
  n_docs = 6, n_tokens = 12;
  write_meta(2);
}

}  // namespace

extern "C" {
const char* np_hip_last_error(void) { return "Invalid argument: the stub said so"; }
int np_hip_abi_version(void) { return NP_ABI_VERSION; }
int64_t np_hip_struct_size(int32_t which) { return which == 0 ? (int64_t)sizeof(np_info) : (int64_t)sizeof(np_stats); }
int np_hip_index_open(const char*, const np_open_opts*, np_index** out) {
  calls.push_back("open");
  *out = (np_index*)&the_index;
  return NP_OK;
}
void np_hip_index_close(np_index*) {}
int np_hip_index_probe_dir(const char*, np_info*) { return NP_ERR_DEVICE_UNAVAILABLE; }
int np_hip_index_info(const np_index*, np_info* out) {
  *out = np_info{};
  out->num_documents = n_docs;
  out->num_embeddings = n_tokens;
  out->embedding_dim = 8;
  out->nbits = 4;
  return NP_OK;
}
// update_index on the directory: the first `join` new documents are appended to the last chunk (rewritten whole, as a v2 NPY
// file: both header versions are read), the rest become chunk 2
int np_hip_index_update_append(const char* index_dir, const float*, const int64_t* lens, int64_t n, int32_t, const np_update_config*,
                               int32_t, np_update_report* report) {
  calls.push_back("update_append");
  CHECK(dir == index_dir);
  enc_lens.assign(lens, lens + n);
  tokens_of(enc_lens, 9, &enc_codes, &enc_res);
  const size_t join = std::min<size_t>(2, (size_t)n);
  int64_t tj = 0, t = 0;
  for (size_t i = 0; i < join; ++i) tj += lens[i];
  for (int64_t i = 0; i < n; ++i) t += lens[i];
  std::vector<int64_t> l1(c1_lens), k1(c1_codes);
  std::vector<uint8_t> r1(c1_res);
  l1.insert(l1.end(), enc_lens.begin(), enc_lens.begin() + join);
  k1.insert(k1.end(), enc_codes.begin(), enc_codes.begin() + tj);
  r1.insert(r1.end(), enc_res.begin(), enc_res.begin() + tj * PD);
  write_chunk(1, l1, k1, r1, 2);
  int64_t chunks = 2;
  if ((size_t)n > join && !forget_a_chunk) {
    write_chunk(2, std::vector<int64_t>(enc_lens.begin() + join, enc_lens.end()), std::vector<int64_t>(enc_codes.begin() + tj, enc_codes.end()),
                std::vector<uint8_t>(enc_res.begin() + tj * PD, enc_res.end()), 1);
    chunks = 3;
  }
  *report = np_update_report{};
  report->first_doc_id = n_docs;
  n_docs += n;       // the directory's counts; the handle's follow in np_hip_index_append
  n_tokens += t;
  write_meta(chunks);
  n_docs -= n;
  n_tokens -= t;
  return NP_OK;
}
int np_hip_index_append(np_index* ix, const int64_t* lens, int64_t n, const int64_t* codes, const uint8_t* res) {
  CHECK(ix == (np_index*)&the_index);
  if (n == 0 && !lens && !codes && !res) {   // the mirror's question before it touches the directory: would the handle refuse?
    calls.push_back("append(nothing)");
    return refuse_handle ? (int)NP_ERR_INVALID_ARGUMENT : (int)NP_OK;
  }
  calls.push_back("append");
  int64_t t = 0;
  for (int64_t i = 0; i < n; ++i) t += lens[i];
  got_lens.assign(lens, lens + n);
  got_codes.assign(codes, codes + t);
  got_res.assign(res, res + t * PD);
  n_docs += n;
  n_tokens += t;
  return NP_OK;
}
int np_hip_index_reserve(np_index* ix, int64_t docs, int64_t tokens) {
  calls.push_back("reserve");
  CHECK(ix == (np_index*)&the_index);
  got_reserve[0] = docs, got_reserve[1] = tokens;
  return docs < 0 ? (int)NP_ERR_INVALID_ARGUMENT : (int)NP_OK;
}
int np_hip_index_capacity(const np_index* ix, int64_t* docs, int64_t* tokens) {
  calls.push_back("capacity");
  CHECK(ix == (const np_index*)&the_index);
  *docs = 77, *tokens = 999;
  return NP_OK;
}
}  // extern "C"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: index_append_check <empty directory>\n");
    return 2;
  }
  dir = argv[1];
  write_base();
  next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(dir);
  CHECK(ix.on_device() && ix.num_documents() == 6);

  // five documents: two join chunk 1, three fill chunk 2; one of them is empty
  std::vector<float> emb(11 * 8, 0.5f);
  next_plaid::Documents docs;
  docs.embeddings = emb.data();
  docs.dim = 8;
  docs.doc_lengths = {4, 1, 0, 3, 3};
  calls.clear();
  np_update_report rep{};
  const std::vector<int64_t> ids = ix.append(docs, {}, 0, &rep);
  CHECK((calls == std::vector<std::string>{"append(nothing)", "update_append", "append"}));
  CHECK((ids == std::vector<int64_t>{6, 7, 8, 9, 10}) && rep.first_doc_id == 6);
  CHECK(got_lens == enc_lens && got_codes == enc_codes && got_res == enc_res);   // what the update wrote, to the byte
  CHECK(got_codes.size() == 11 && ix.num_documents() == 11 && ix.num_embeddings() == 23);

  // an update without documents appends nothing and still passes
  docs.doc_lengths.clear();
  calls.clear();
  CHECK(ix.append(docs).empty() && ix.num_documents() == 11);
  CHECK((calls == std::vector<std::string>{"append(nothing)", "update_append", "append(nothing)"}));

  // a directory whose chunk files do not hold what metadata.json counts: refused before the handle is touched
  docs.doc_lengths = {1, 1, 5};
  forget_a_chunk = true;
  calls.clear();
  try {
    (void)ix.append(docs);
    CHECK(!"a short directory was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::IndexLoad && (calls == std::vector<std::string>{"append(nothing)", "update_append"}));
  }
  // the directory is now ahead of the handle (14 documents against 11): refused before the library is called at all
  forget_a_chunk = false;
  calls.clear();
  try {
    (void)ix.append(docs);
    CHECK(!"a handle behind its directory was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::IndexLoad && calls.empty());
  }
  // a handle the library would refuse (a shard, lists that do not ascend) is refused BEFORE the directory is rewritten
  n_docs = 14, n_tokens = 30;   // (the handle reloaded: current again)
  ix.reload();
  refuse_handle = true;
  calls.clear();
  try {
    (void)ix.append(docs);
    CHECK(!"the library's refusal was swallowed");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config && (calls == std::vector<std::string>{"append(nothing)"}));
  }
  refuse_handle = false;

  // append_arrays, reserve, capacity: the caller's arrays and figures as they are
  const std::vector<int64_t> lens{2, 1}, codes{3, 4, 5};
  const std::vector<uint8_t> res(3 * PD, 7);
  const int64_t first = (int64_t)ix.num_documents();
  CHECK((ix.append_arrays(lens, codes.data(), res.data()) == std::vector<int64_t>{first, first + 1}));
  CHECK(got_lens == lens && got_codes == codes && got_res == res && (int64_t)ix.num_documents() == first + 2);
  ix.reserve(1000, 300000);
  CHECK(got_reserve[0] == 1000 && got_reserve[1] == 300000);
  CHECK((ix.capacity() == std::pair<int64_t, int64_t>{77, 999}));
  try {
    ix.reserve(-1, 0);
    CHECK(!"the library's refusal was swallowed");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config);
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
