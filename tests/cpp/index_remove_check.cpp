// What next_plaid.hpp's MmapIndex::remove / remove_ids hand np_hip_index_delete and np_hip_index_remove: the caller's ids as
// they are, the directory first and the handle behind it, and the refusals that happen before the directory is touched.  With
// the host compiler alone: the np_hip_* entries are recording stubs in this translation unit (no library is linked).
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
std::string dir;
std::vector<std::string> calls;
int64_t n_docs = 0, dir_docs = 0;   // what the stub handle and the directory hold
std::vector<int64_t> got_delete, got_remove;
bool refuse_handle = false, handle_loses_one_less = false;

void write_meta() {
  const std::string s = "{\n  \"num_chunks\": 1,\n  \"nbits\": 4,\n  \"num_partitions\": 16,\n  \"num_embeddings\": " +
                        std::to_string((long long)dir_docs * 2) + ",\n  \"avg_doclen\": 2.0,\n  \"num_documents\": " +
                        std::to_string((long long)dir_docs) + ",\n  \"embedding_dim\": 8\n}";
  std::FILE* f = std::fopen((dir + "/metadata.json").c_str(), "wb");
  if (!f || std::fwrite(s.data(), 1, s.size(), f) != s.size()) {
    std::printf("cannot write metadata.json\n");
    std::exit(2);
  }
  std::fclose(f);
}
// the distinct ids inside [0, n)
int64_t distinct_in_range(const std::vector<int64_t>& ids, int64_t n) {
  std::vector<char> hit((size_t)n, 0);
  int64_t c = 0;
  for (int64_t id : ids)
    if (id >= 0 && id < n && !hit[(size_t)id]) hit[(size_t)id] = 1, ++c;
  return c;
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
  out->num_embeddings = n_docs * 2;
  out->embedding_dim = 8;
  out->nbits = 4;
  return NP_OK;
}
int np_hip_index_delete(const char* index_dir, const int64_t* ids, int64_t n, int64_t* out_deleted) {
  calls.push_back("delete");
  CHECK(dir == index_dir);
  got_delete.assign(ids, ids + n);
  const int64_t c = distinct_in_range(got_delete, dir_docs);
  dir_docs -= c;
  write_meta();
  if (out_deleted) *out_deleted = c;
  return NP_OK;
}
int np_hip_index_remove(np_index* ix, const int64_t* ids, int64_t n, int64_t* out_removed) {
  CHECK(ix == (np_index*)&the_index);
  if (n == 0 && !ids && !out_removed) {   // the mirror's question before it touches the directory: would the handle refuse?
    calls.push_back("remove(nothing)");
    return refuse_handle ? (int)NP_ERR_INVALID_ARGUMENT : (int)NP_OK;
  }
  calls.push_back("remove");
  got_remove.assign(ids, ids + n);
  const int64_t c = distinct_in_range(got_remove, n_docs) - (handle_loses_one_less ? 1 : 0);
  n_docs -= c;
  if (out_removed) *out_removed = c;
  return NP_OK;
}
}  // extern "C"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: index_remove_check <empty directory>\n");
    return 2;
  }
  dir = argv[1];
  n_docs = dir_docs = 20;
  write_meta();
  next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(dir);
  CHECK(ix.on_device() && ix.num_documents() == 20);

  // the directory first, then the handle, both with the caller's ids as they are: out of range and twice included
  const std::vector<int64_t> ids{3, 17, 3, -1, 20, 5};
  calls.clear();
  CHECK(ix.remove(ids) == 3);
  CHECK((calls == std::vector<std::string>{"remove(nothing)", "delete", "remove"}));
  CHECK(got_delete == ids && got_remove == ids && ix.num_documents() == 17 && ix.num_embeddings() == 34 && dir_docs == 17);

  // nothing in range: both are still asked, nothing changes
  calls.clear();
  CHECK(ix.remove({-4, 17}) == 0 && ix.num_documents() == 17);
  CHECK((calls == std::vector<std::string>{"remove(nothing)", "delete", "remove"}));

  // remove_ids: the handle alone
  calls.clear();
  CHECK(ix.remove_ids({0, 16, 16}) == 2 && ix.num_documents() == 15 && dir_docs == 17);
  CHECK((calls == std::vector<std::string>{"remove"}) && (got_remove == std::vector<int64_t>{0, 16, 16}));

  // the directory is now ahead of the handle (17 documents against 15): refused before the library is called at all
  calls.clear();
  try {
    (void)ix.remove({1});
    CHECK(!"a handle that is not current was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::IndexLoad && calls.empty() && dir_docs == 17);
  }
  // a handle the library would refuse (a shard) is refused BEFORE the directory is rewritten
  n_docs = 17;
  ix.reload();
  refuse_handle = true;
  calls.clear();
  try {
    (void)ix.remove({1});
    CHECK(!"the library's refusal was swallowed");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config && (calls == std::vector<std::string>{"remove(nothing)"}) && dir_docs == 17);
  }
  refuse_handle = false;
  // a handle that lost another number of documents than its directory is reported, not served
  handle_loses_one_less = true;
  try {
    (void)ix.remove({1, 2});
    CHECK(!"a handle that disagrees with its directory was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::IndexLoad);
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
