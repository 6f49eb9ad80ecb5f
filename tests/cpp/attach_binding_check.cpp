// What next_plaid.hpp hands np_hip_index_remove_keep, np_hip_index_append_rows, np_hip_index_get_column and
// np_hip_index_get_groups: which entry keep_attachments and rows reach, the argument values, and the refusals that happen before
// the library or the directory is touched.  With the host compiler alone: the np_hip_* entries are recording stubs in this
// translation unit (no library is linked).  Built with -fsanitize=address,undefined.  argv[1] = an empty directory to work in.
#include <cstdio>
#include <cstring>
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
int64_t n_docs = 0, dir_docs = 0, handle_groups = 0;
std::vector<int64_t> got_ids;
struct GotRows {
  int64_t n_docs = 0, n_groups = 0;
  int32_t n_cols = 0;
  std::vector<int32_t> types, groups, remap1;
  std::vector<int64_t> col0;
  bool remap_null = true, remap0_null = true, groups_null = true;
} got;
bool refuse_rows = false;

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

}  // namespace

extern "C" {
const char* np_hip_last_error(void) { return "Invalid argument: the stub said so"; }
int np_hip_abi_version(void) { return NP_ABI_VERSION; }
int64_t np_hip_struct_size(int32_t which) { return which == 0 ? (int64_t)sizeof(np_info) : (int64_t)sizeof(np_stats); }
int np_hip_index_open(const char*, const np_open_opts*, np_index** out) {
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
  out->shard_doc_end = n_docs;
  return NP_OK;
}
int np_hip_index_delete(const char*, const int64_t*, int64_t n, int64_t* out_deleted) {
  calls.push_back("delete");
  dir_docs -= n;
  write_meta();
  if (out_deleted) *out_deleted = n;
  return NP_OK;
}
int np_hip_index_remove(np_index*, const int64_t*, int64_t, int64_t*) {
  calls.push_back("remove");
  return NP_OK;
}
int np_hip_index_remove_keep(np_index* ix, const int64_t* ids, int64_t n, int64_t* out_removed) {
  CHECK(ix == (np_index*)&the_index);
  if (n == 0 && !ids && !out_removed) {
    calls.push_back("remove_keep(nothing)");
    return NP_OK;
  }
  calls.push_back("remove_keep");
  got_ids.assign(ids, ids + n);
  n_docs -= n;
  if (out_removed) *out_removed = n;
  return NP_OK;
}
int np_hip_index_append(np_index*, const int64_t*, int64_t, const int64_t*, const uint8_t*) {
  calls.push_back("append");
  return NP_OK;
}
int np_hip_index_update_append(const char*, const float*, const int64_t*, int64_t, int32_t, const np_update_config*, int32_t,
                               np_update_report*) {
  calls.push_back("update_append");   // the directory: never reached by the refusals below
  return NP_ERR_INVALID_ARGUMENT;
}
int64_t np_hip_index_group_count(const np_index*) {
  calls.push_back("group_count");
  return handle_groups;
}
int np_hip_index_append_rows(np_index* ix, const int64_t* lens, int64_t n, const int64_t*, const uint8_t*, const np_column* cols,
                             int32_t n_cols, const int32_t* const* remap, const int32_t* groups, int64_t n_groups) {
  CHECK(ix == (np_index*)&the_index);
  calls.push_back(n == 0 && !lens ? "append_rows(nothing)" : "append_rows");
  if (refuse_rows) return NP_ERR_INVALID_ARGUMENT;
  got = GotRows{};
  got.n_docs = n, got.n_cols = n_cols, got.n_groups = n_groups;
  for (int32_t c = 0; c < n_cols; ++c) got.types.push_back(cols[c].type);
  if (n_cols > 0 && n > 0) got.col0.assign((const int64_t*)cols[0].data, (const int64_t*)cols[0].data + n);
  got.remap_null = remap == nullptr;
  if (remap) {
    got.remap0_null = remap[0] == nullptr;
    if (n_cols > 1 && remap[1]) got.remap1.assign(remap[1], remap[1] + 2);
  }
  got.groups_null = groups == nullptr;
  if (groups) got.groups.assign(groups, groups + n);
  n_docs += n;
  return NP_OK;
}
int np_hip_index_get_column(const np_index*, int32_t column, void* data, uint8_t* valid, int32_t* type, int32_t* has_valid) {
  calls.push_back(data ? "get_column" : "get_column(shape)");
  CHECK(column == 1);
  *type = NP_COL_CODE, *has_valid = 1;
  for (int64_t d = 0; data && d < n_docs; ++d) ((int32_t*)data)[d] = (int32_t)d, valid[d] = (uint8_t)(d & 1);
  return NP_OK;
}
int np_hip_index_get_groups(const np_index*, int32_t* out) {
  calls.push_back("get_groups");
  for (int64_t d = 0; d < n_docs; ++d) out[d] = (int32_t)(d % 3);
  return NP_OK;
}
}  // extern "C"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: attach_binding_check <empty directory>\n");
    return 2;
  }
  using Calls = std::vector<std::string>;
  dir = argv[1];
  n_docs = dir_docs = 20;
  write_meta();
  next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(dir);
  CHECK(ix.on_device() && ix.num_documents() == 20);

  // keep_attachments picks the entry, for the handle alone and for the question before the directory is touched
  const std::vector<int64_t> ids{3, 17};
  calls.clear();
  CHECK(ix.remove_ids(ids, true) == 2 && got_ids == ids && ix.num_documents() == 18);
  CHECK((calls == Calls{"remove_keep"}));
  calls.clear();
  CHECK(ix.remove_ids(ids, false) == 0);
  CHECK((calls == Calls{"remove"}));
  n_docs = 20;
  ix.reload();
  calls.clear();
  CHECK(ix.remove(ids, true) == 2 && dir_docs == 18 && ix.num_documents() == 18);
  CHECK((calls == Calls{"remove_keep(nothing)", "delete", "remove_keep"}));

  // the read-back entries: the shape first, then the rows
  calls.clear();
  const auto col = ix.get_column(1);
  CHECK((calls == Calls{"get_column(shape)", "get_column"}) && col.type == NP_COL_CODE && col.has_valid);
  CHECK(col.data.size() == 18 * 4 && col.valid.size() == 18 && col.valid[1] == 1 && col.valid[2] == 0);
  int32_t v = 0;
  std::memcpy(&v, col.data.data() + 4 * 17, 4);
  CHECK(v == 17);
  calls.clear();
  CHECK(ix.get_groups().size() == 18 && ix.get_groups()[5] == 2);

  // append_arrays with rows: the spans, the remap table and the groups as they are
  const std::vector<int64_t> lens{2, 1, 3}, codes{1, 2, 3, 4, 5, 6}, a{7, 8, 9};
  const std::vector<uint8_t> res(6 * 4, 0);
  const std::vector<int32_t> c{0, 2, 1}, remap{0, 2};
  next_plaid::MmapIndex::AppendedRows rows;
  rows.columns = {next_plaid::ColumnSpan::i64(a.data(), 3), next_plaid::ColumnSpan::codes(c.data(), 3)};
  rows.code_remap = {nullptr, remap.data()};
  rows.groups = {4, 0, 4};
  rows.n_groups = 5;
  calls.clear();
  const std::vector<int64_t> fresh = ix.append_arrays(lens, codes.data(), res.data(), rows);
  CHECK((calls == Calls{"append_rows"}) && (fresh == std::vector<int64_t>{18, 19, 20}) && ix.num_documents() == 21);
  CHECK(got.n_docs == 3 && got.n_cols == 2 && got.n_groups == 5 && (got.types == std::vector<int32_t>{NP_COL_I64, NP_COL_CODE}));
  CHECK(got.col0 == a && !got.remap_null && got.remap0_null && got.remap1 == remap && got.groups == rows.groups);
  // no remap, no groups: NULL pointers
  rows.code_remap.clear();
  rows.groups.clear();
  (void)ix.append_arrays(lens, codes.data(), res.data(), rows);
  CHECK(got.remap_null && got.groups_null && got.n_cols == 2);
  // without rows the plain entry
  calls.clear();
  (void)ix.append_arrays(lens, codes.data(), res.data());
  CHECK((calls == Calls{"append"}));

  // refused before the library is touched: a span of another length, a remap list of another length, groups of another length
  calls.clear();
  rows.columns[0].size = 2;
  try {
    (void)ix.append_arrays(lens, codes.data(), res.data(), rows);
    CHECK(!"a short column was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Shape && calls.empty());
  }
  rows.columns[0].size = 3;
  rows.code_remap = {nullptr};
  try {
    (void)ix.append_arrays(lens, codes.data(), res.data(), rows);
    CHECK(!"a short remap list was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Shape && calls.empty());
  }
  rows.code_remap.clear();
  rows.groups = {1};
  try {
    (void)ix.append_arrays(lens, codes.data(), res.data(), rows);
    CHECK(!"a short group list was accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Shape && calls.empty());
  }

  // append() with rows asks the library about the handle AND the rows before the directory is touched
  next_plaid::Documents docs;
  const std::vector<float> emb(3 * 8, 0.f);
  docs.embeddings = emb.data(), docs.doc_lengths = {1, 1, 1}, docs.dim = 8;
  rows.groups = {0, 1, 2};
  dir_docs = n_docs;
  write_meta();
  handle_groups = 0;   // groups for a handle without: refused after the one question, the directory as it was
  calls.clear();
  try {
    (void)ix.append_with_rows(docs, rows);
    CHECK(!"groups for a handle without groups were accepted");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config && (calls == Calls{"group_count"}));
  }
  // no documents, no groups: the rule does not apply, the library is asked (and append(docs, {}) still means a default config)
  next_plaid::Documents none;
  none.embeddings = emb.data(), none.dim = 8;
  next_plaid::MmapIndex::AppendedRows bare;
  bare.columns = {next_plaid::ColumnSpan::i64(a.data(), 0), next_plaid::ColumnSpan::codes(c.data(), 0)};
  handle_groups = 3;
  refuse_rows = true;
  calls.clear();
  try {
    (void)ix.append_with_rows(none, bare);
    CHECK(!"the library's refusal was swallowed");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config && (calls == Calls{"append_rows(nothing)"}));
  }
  if (false) (void)ix.append(docs, {});   // compiles: one append takes a braced config
  handle_groups = 3;
  refuse_rows = true;
  calls.clear();
  try {
    (void)ix.append_with_rows(docs, rows);
    CHECK(!"the library's refusal of the rows was swallowed");
  } catch (const next_plaid::Error& e) {
    CHECK(e.kind == next_plaid::Error::Config && (calls == Calls{"group_count", "append_rows(nothing)"}));
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
