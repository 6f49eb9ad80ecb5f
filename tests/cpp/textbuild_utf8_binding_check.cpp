// What next_plaid.hpp's keyword-index entries put into np_text_build_opts.unicode_table -- with the host compiler alone.
// np_hip_text_build is a recording stub in this translation unit (no library is linked), the entries around it answer just
// enough for the callers to go on.  Without a table the pointer is NULL and the length 0; with one, every overload hands on
// the caller's vector, its pointer and its length.  The struct and the ABI version are what they were.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

struct stub {
  int dummy;
};
stub the_index, the_batch, the_result;
std::vector<np_text_build_opts> seen;   // the options of every np_hip_text_build
std::vector<int64_t> fallback;
int failed = 0;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

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
  out->device = 3;
  out->num_documents = 5;
  out->embedding_dim = 8;
  out->nbits = 4;
  return NP_OK;
}
int np_hip_text_build(int32_t, const uint8_t*, const int64_t*, int64_t n, const np_text_build_opts* opts, np_text_build** out_build,
                      np_text_build_report* report) {
  seen.push_back(*opts);
  *out_build = (np_text_build*)&the_batch;
  *report = np_text_build_report{};
  report->n_docs = n;
  report->n_fallback = (int64_t)fallback.size();
  return NP_OK;
}
int np_hip_text_build_fallback(const np_text_build*, int64_t* ids, int64_t*) {
  for (size_t i = 0; i < fallback.size(); ++i) ids[i] = fallback[i];
  return NP_OK;
}
int np_hip_text_build_add(np_text_build*, const uint8_t*, const int64_t*, int64_t, const int32_t*, const int64_t*, const int32_t*, int64_t) {
  return NP_OK;
}
int np_hip_text_build_sizes(np_text_build*, int64_t* n_terms, int64_t* term_bytes, int64_t* n_inst, int64_t* rows) {
  if (n_terms) *n_terms = 1;
  if (term_bytes) *term_bytes = 2;
  if (n_inst) *n_inst = 1;
  if (rows) *rows = 5;
  return NP_OK;
}
int np_hip_text_build_fetch(const np_text_build*, uint8_t* tb, int64_t* tbo, int64_t* toff, int64_t* idoc, int32_t* ipos) {
  memcpy(tb, "zz", 2);
  tbo[0] = 0, tbo[1] = 2;
  if (toff) toff[0] = 0, toff[1] = 1;
  if (idoc) idoc[0] = 0;
  if (ipos) ipos[0] = 0;
  return NP_OK;
}
void np_hip_text_build_free(np_text_build*) {}
int np_hip_text_build_merge(int32_t, const np_text_index*, const uint8_t*, const int64_t*, const int64_t*, int64_t, const np_text_build*,
                            const int64_t*, int64_t, const np_text_merge_opts*, np_text_build** out_build, np_text_merge_report* report) {
  *out_build = (np_text_build*)&the_result;
  *report = np_text_merge_report{};
  return NP_OK;
}
int np_hip_index_set_text_build(np_index*, np_text_build*) { return NP_OK; }
int np_hip_index_text_sizes(const np_index*, int64_t* n_terms, int64_t*, int64_t*, int64_t*, int64_t*) {
  if (n_terms) *n_terms = 1;
  return NP_OK;
}
int np_hip_index_text_merge(const np_index*, const uint8_t*, const int64_t*, const int64_t*, int64_t, const np_text_build*, const int64_t*,
                            int64_t, const np_text_merge_opts*, np_text_build** out_build, np_text_merge_report* report) {
  *out_build = (np_text_build*)&the_result;
  *report = np_text_merge_report{};
  return NP_OK;
}
}

using namespace next_plaid;

int main(int argc, char** argv) {
  static_assert(NP_ABI_VERSION == 6, "the ABI version stays 6");
  static_assert(sizeof(np_text_build_opts) == 48, "np_text_build_opts does not grow");
  static_assert(sizeof(np_text_build_report) == 136 && sizeof(np_text_merge_opts) == 32, "the report and the merge's options stay");
  static_assert(offsetof(np_text_build_opts, unicode_table) == 24 && offsetof(np_text_build_opts, unicode_table_len) == 32 &&
                    offsetof(np_text_build_opts, reserved) == 40,
                "the table takes two of the three reserved words");
  const std::vector<std::string> texts = {"caf\xC3\xA9", "", "cd"};
  std::vector<uint32_t> table((size_t)2 * 65536, 0u);   // the stub does not read it.  NOT const: a table the caller holds as a
  const std::vector<uint32_t>& ctable = table;          // plain vector must select the same overloads as a const one
  auto plain = [&](int32_t tokenizer, int32_t cap) {
    const np_text_build_opts& o = seen.back();
    return o.unicode_table == nullptr && o.unicode_table_len == 0 && o.reserved[0] == 0 && o.tokenizer == tokenizer && o.max_token_bytes == cap;
  };
  auto with = [&](int32_t tokenizer, int32_t cap) {
    const np_text_build_opts& o = seen.back();
    return o.unicode_table == table.data() && o.unicode_table_len == 131072 && o.reserved[0] == 0 && o.tokenizer == tokenizer &&
           o.max_token_bytes == cap && o.hash_bits == 0 && o.tile_bytes == 0 && o.workspace_bytes == 0;
  };
  auto tokenize = [](const std::vector<int64_t>&) { return TextInstances{}; };
  BuiltTextIndex base;
  base.terms = {"zz"};
  base.term_offsets = {0, 1};
  base.inst_doc = {0};
  base.inst_pos = {0};
  base.n_rows = 5;
  TextUpdate u;
  u.new_texts = {"na\xC3\xAFve"};
  MmapIndex ix = MmapIndex::load("unused");
  ResidentTextIndex cur;
  cur.terms = {"zz"};
  cur.n_rows = 5;

  // without a table: NULL, as before
  build_text_index(texts, Tokenizer::Unicode61, 0, 9);
  CHECK(plain(NP_TOK_UNICODE61, 9));
  build_text_index(texts, Tokenizer::Trigram, tokenize);
  CHECK(plain(NP_TOK_TRIGRAM, 0));
  update_text_index(base, u);
  CHECK(plain(NP_TOK_UNICODE61, 0));
  update_text_index(base, u, Tokenizer::Unicode61, tokenize);
  CHECK(plain(NP_TOK_UNICODE61, 0));
  build_text_resident(ix, texts);
  CHECK(plain(NP_TOK_UNICODE61, 0));
  update_text_resident(ix, cur, u);
  CHECK(plain(NP_TOK_UNICODE61, 0));
  CHECK(seen.size() == 6);

  // with one: the caller's vector through every overload
  build_text_index(texts, table, Tokenizer::Unicode61, 0, 9);
  CHECK(with(NP_TOK_UNICODE61, 9));
  build_text_index(texts, table);
  CHECK(with(NP_TOK_UNICODE61, 0));
  fallback = {1};
  int asked = 0;
  build_text_index(texts, table, Tokenizer::Unicode61, [&](const std::vector<int64_t>& ids) {
    ++asked;
    CHECK(ids == std::vector<int64_t>{1});
    return TextInstances{};
  });
  CHECK(with(NP_TOK_UNICODE61, 0) && asked == 1);
  fallback.clear();
  build_text_index(texts, table, Tokenizer::Trigram);   // handed on; the library ignores it for trigram
  CHECK(with(NP_TOK_TRIGRAM, 0));
  update_text_index(base, u, table);
  CHECK(with(NP_TOK_UNICODE61, 0));
  update_text_index(base, u, table, Tokenizer::Unicode61, tokenize, 0, 300);
  CHECK(with(NP_TOK_UNICODE61, 300));
  build_text_resident(ix, texts, table, Tokenizer::Unicode61, 77);
  CHECK(with(NP_TOK_UNICODE61, 77));
  update_text_resident(ix, cur, u, table);
  CHECK(with(NP_TOK_UNICODE61, 0));
  int stepped = 0;
  update_text_resident(ix, cur, u, table, [&] { ++stepped; }, Tokenizer::Unicode61, 12);
  CHECK(with(NP_TOK_UNICODE61, 12) && stepped == 1);
  CHECK(seen.size() == 15);
  // ... with the caller's tokenizer for what still falls back in UTF-8 mode
  fallback = {0};
  asked = 0;
  auto counting = [&](const std::vector<int64_t>& ids) {
    ++asked;
    CHECK(ids == std::vector<int64_t>{0});
    return TextInstances{};
  };
  const ResidentTextIndex rb = build_text_resident(ix, texts, table, Tokenizer::Unicode61, counting, 31);
  CHECK(with(NP_TOK_UNICODE61, 31) && asked == 1 && rb.fallback_docs == std::vector<int64_t>{0});
  const ResidentTextIndex ru = update_text_resident(ix, cur, u, table, [&] { ++stepped; }, Tokenizer::Unicode61, counting, 32);
  CHECK(with(NP_TOK_UNICODE61, 32) && asked == 2 && stepped == 2 && ru.fallback_docs == std::vector<int64_t>{0});
  fallback.clear();
  CHECK(seen.size() == 17);
  // the same through a const reference and through a temporary
  build_text_index(texts, ctable);
  CHECK(with(NP_TOK_UNICODE61, 0));
  update_text_index(base, u, ctable);
  CHECK(with(NP_TOK_UNICODE61, 0));
  build_text_resident(ix, texts, ctable);
  CHECK(with(NP_TOK_UNICODE61, 0));
  update_text_resident(ix, cur, u, ctable);
  CHECK(with(NP_TOK_UNICODE61, 0));
  update_text_resident(ix, cur, u, ctable, [&] { ++stepped; });
  CHECK(with(NP_TOK_UNICODE61, 0) && stepped == 3);
  update_text_resident(ix, cur, u, std::vector<uint32_t>((size_t)65536, 0u));
  CHECK(seen.back().unicode_table != nullptr && seen.back().unicode_table_len == 65536);
  CHECK(seen.size() == 23);

  // a table file as numpy's tofile writes it: raw little-endian uint32
  if (argc > 1) {
    std::vector<uint32_t> t = load_unicode_table(argv[1]);   // held as the header's comment says, and passed on
    CHECK(t.size() == 131072 && t['A'] == ((1u << 30) | 'a') && t[' '] == 0 && (t[0x301] >> 30) == 2 && (t[0xC9] & 0x1FFFFF) == 'e');
    build_text_index(texts, t);
    CHECK(seen.back().unicode_table == t.data() && seen.back().unicode_table_len == 131072);
    update_text_resident(ix, cur, u, t);
    CHECK(seen.back().unicode_table == t.data() && seen.back().unicode_table_len == 131072);
  }
  bool thrown = false;
  try {
    load_unicode_table("/nonexistent/table.u32");
  } catch (const Error&) {
    thrown = true;
  }
  CHECK(thrown);
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
