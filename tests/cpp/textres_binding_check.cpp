// What next_plaid.hpp's build_text_resident / update_text_resident / get_text / get_text_layout hand the library, in which
// order, and what they free -- with the host compiler alone.  The np_hip_* entries they reach are recording stubs in this
// translation unit (no library is linked).  Built with -fsanitize=address,undefined: an array the header sized too small is
// an error there.
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
std::vector<std::string> calls;
std::vector<int64_t> fallback;
std::string got_bytes, got_base_terms;
std::vector<int64_t> got_offsets, got_remap, got_ids, got_base_tbo;
int64_t got_rows_out = -1, held_terms = 2, n_docs = 5;
const np_text_build* got_delta = nullptr;
const np_text_build* installed = nullptr;
int got_device = -1, failed = 0;
std::string fail_entry;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

int note(const char* name) {
  calls.push_back(name);
  return fail_entry == name ? (int)NP_ERR_INVALID_ARGUMENT : (int)NP_OK;
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
  out->device = 3;
  out->num_documents = n_docs;
  out->embedding_dim = 8;
  out->nbits = 4;
  return NP_OK;
}

int np_hip_text_build(int32_t device, const uint8_t* bytes, const int64_t* offsets, int64_t n, const np_text_build_opts*,
                      np_text_build** out_build, np_text_build_report* report) {
  got_device = device;
  got_offsets.assign(offsets, offsets + n + 1);
  got_bytes.assign((const char*)bytes, (size_t)offsets[n]);
  *out_build = (np_text_build*)&the_batch;
  *report = np_text_build_report{};
  report->n_docs = n;
  report->n_fallback = (int64_t)fallback.size();
  return note("build");
}
int np_hip_text_build_fallback(const np_text_build*, int64_t* ids, int64_t*) {
  for (size_t i = 0; i < fallback.size(); ++i) ids[i] = fallback[i];
  return note("fallback");
}
int np_hip_text_build_add(np_text_build* b, const uint8_t*, const int64_t*, int64_t, const int32_t*, const int64_t*, const int32_t*, int64_t) {
  CHECK(b == (np_text_build*)&the_batch);
  return note("add");
}
int np_hip_text_build_sizes(np_text_build* b, int64_t* n_terms, int64_t* term_bytes, int64_t* n_inst, int64_t* rows) {
  if (!n_terms) {   // only finalised
    CHECK(!term_bytes && !n_inst && !rows);
    return note(b == (np_text_build*)&the_batch ? "sizes(batch)" : "sizes(result)");
  }
  CHECK(b == installed);   // the sizes of a build are read after it was installed
  *n_terms = 1, *term_bytes = 2, *n_inst = 2, *rows = 7;
  return note("sizes");
}
int np_hip_text_build_fetch(const np_text_build* b, uint8_t* tb, int64_t* tbo, int64_t* toff, int64_t* idoc, int32_t* ipos) {
  CHECK(b == installed);
  CHECK(!toff && !idoc && !ipos);   // no instance array crosses the bus
  memcpy(tb, "zz", 2);
  tbo[0] = 0, tbo[1] = 2;
  return note("fetch(vocabulary)");
}
void np_hip_text_build_free(np_text_build* b) {
  calls.push_back(!b ? "free(null)" : b == (np_text_build*)&the_batch ? "free(batch)" : "free(result)");
}

int np_hip_index_set_text_build(np_index* ix, np_text_build* b) {
  CHECK(ix == (np_index*)&the_index);
  const int rc = note("install");
  if (rc == NP_OK) installed = b;
  return rc;
}
int np_hip_index_text_sizes(const np_index* ix, int64_t* n_terms, int64_t* n_post, int64_t* n_inst, int64_t* rows, int64_t* docs) {
  CHECK(ix == (const np_index*)&the_index);
  if (n_terms) *n_terms = held_terms;
  if (n_post) *n_post = 3;
  if (n_inst) *n_inst = 4;
  if (rows) *rows = 5;
  if (docs) *docs = n_docs;
  return note("text_sizes");
}
int np_hip_index_text_merge(const np_index* ix, const uint8_t* tb, const int64_t* tbo, const int64_t* remap, int64_t n_remap,
                            const np_text_build* delta, const int64_t* delta_ids, int64_t n_rows_out, const np_text_merge_opts* opts,
                            np_text_build** out_build, np_text_merge_report* report) {
  CHECK(ix == (const np_index*)&the_index);
  got_base_tbo.assign(tbo, tbo + held_terms + 1);
  got_base_terms.assign((const char*)tb, (size_t)tbo[held_terms]);
  got_remap.assign(remap, remap + n_remap);
  got_delta = delta;
  const int64_t m = delta ? (int64_t)got_offsets.size() - 1 : 0;
  got_ids.clear();
  if (m > 0) got_ids.assign(delta_ids, delta_ids + m);
  got_rows_out = n_rows_out;
  CHECK(opts && opts->workspace_bytes == 0 && report);
  *report = np_text_merge_report{};
  report->n_instances = 2;
  const int rc = note("merge");
  if (rc == NP_OK) *out_build = (np_text_build*)&the_result;
  return rc;
}
int np_hip_index_get_text(const np_index*, int64_t* toff, int64_t* idoc, int32_t* ipos) {
  for (int64_t k = 0; k <= held_terms; ++k) toff[k] = 2 * k;
  for (int i = 0; i < 4; ++i) idoc[i] = i, ipos[i] = (int32_t)(10 + i);
  return note("get_text");
}
int np_hip_index_get_text_layout(const np_index*, int64_t* post_off, int32_t* post_doc, int32_t* post_tf, int64_t* post_first, int32_t* doc_len) {
  for (int64_t k = 0; k <= held_terms; ++k) post_off[k] = k;
  for (int i = 0; i < 3; ++i) post_doc[i] = i, post_tf[i] = 1, post_first[i] = i;
  for (int64_t d = 0; d < n_docs; ++d) doc_len[d] = (int32_t)d;
  return note("get_text_layout");
}
int np_hip_index_remove(np_index*, const int64_t*, int64_t, int64_t*) { return note("remove"); }
int np_hip_index_remove_keep(np_index*, const int64_t*, int64_t n, int64_t* out) {
  const int rc = note("remove_keep");
  if (rc == NP_OK) *out = n, n_docs -= n;
  return rc;
}
}

using namespace next_plaid;
using Names = std::vector<std::string>;
using V = std::vector<int64_t>;

int main() {
  MmapIndex ix = MmapIndex::load("unused");
  const Names install = {"sizes(result)", "install", "sizes", "fetch(vocabulary)"};
  auto plus = [](Names a, const Names& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
  };
  {   // build -> fallback -> sizes -> install; only the vocabulary is fetched
    calls.clear();
    const ResidentTextIndex r = build_text_resident(ix, {"ab cd", "", "cd"}, Tokenizer::Unicode61, 77);
    CHECK((calls == Names{"build", "fallback", "sizes(batch)", "install", "sizes", "fetch(vocabulary)", "free(batch)"}));
    CHECK(got_bytes == "ab cdcd" && (got_offsets == V{0, 5, 5, 7}) && got_device == 3);
    CHECK(installed == (np_text_build*)&the_batch && (r.terms == Names{"zz"}) && r.n_rows == 7 && r.n_instances == 2);
  }
  {   // a fallback document without a tokenize is an error before the install; with one its instances are added once
    fallback = {1};
    calls.clear();
    bool thrown = false;
    try {
      (void)build_text_resident(ix, {"ab", "caf\xc3\xa9", "cd"});
    } catch (const Error& e) {
      thrown = std::string(e.what()).find("document 1 is not reproduced on the device") != std::string::npos;
    }
    CHECK(thrown && (calls == Names{"build", "fallback", "free(batch)"}));
    calls.clear();
    int asked = 0;
    const ResidentTextIndex r = build_text_resident(ix, {"ab", "caf\xc3\xa9", "cd"}, Tokenizer::Unicode61, [&](const V& ids) {
      ++asked;
      CHECK((ids == V{1}));
      TextInstances t;
      t.terms = {"cafe"};
      t.inst_term = {0};
      t.inst_doc = {1};
      t.inst_pos = {0};
      return t;
    });
    CHECK(asked == 1 && (calls == Names{"build", "fallback", "add", "sizes(batch)", "install", "sizes", "fetch(vocabulary)", "free(batch)"}));
    CHECK((r.fallback_docs == V{1}));
    fallback.clear();
  }
  ResidentTextIndex cur;   // rows 0..4 with the vocabulary "ab", "cd"
  cur.terms = {"ab", "cd"};
  cur.n_rows = 5;
  {   // merge -> install, with the argument values; batch first, then the result is freed
    TextUpdate u;
    u.new_texts = {"zz", "ab"};
    u.delete_ids = {1};
    u.replace = {{3, "three"}};
    calls.clear();
    const ResidentTextIndex r = update_text_resident(ix, cur, u);
    CHECK((calls == plus(plus({"text_sizes", "build", "fallback", "sizes(batch)", "merge", "free(batch)"}, install), {"free(result)"})));
    CHECK(got_bytes == "threezzab" && got_base_terms == "abcd" && (got_base_tbo == V{0, 2, 4}));
    CHECK((got_remap == V{0, -1, 1, -1, 3}) && (got_ids == V{2, 4, 5}) && got_rows_out == 6 && got_delta == (np_text_build*)&the_batch);
    CHECK(installed == (np_text_build*)&the_result && (r.terms == Names{"zz"}) && r.merge_report.n_instances == 2);
  }
  {   // the vector call runs between the merge and the install
    TextUpdate u;
    u.delete_ids = {0, 4};
    calls.clear();
    int64_t removed = 0;
    (void)update_text_resident(ix, cur, u, [&] { removed = ix.remove_ids({0, 4}, /*keep_attachments=*/true); });
    CHECK(removed == 2 && (calls == plus(plus({"text_sizes", "merge", "free(null)", "remove_keep"}, install), {"free(result)"})));
    CHECK((got_remap == V{-1, 0, 1, 2, -1}) && got_ids.empty() && got_rows_out == 3 && got_delta == nullptr);
    n_docs = 5;
  }
  {   // a refused vector call: the handle is not installed on and the merge's result is freed
    TextUpdate u;
    u.delete_ids = {2};
    fail_entry = "remove_keep";
    calls.clear();
    bool thrown = false;
    try {
      (void)update_text_resident(ix, cur, u, [&] { (void)ix.remove_ids({2}, true); });
    } catch (const Error&) {
      thrown = true;
    }
    CHECK(thrown && (calls == Names{"text_sizes", "merge", "free(null)", "remove_keep", "free(result)"}));
    fail_entry.clear();
  }
  {   // a refused merge frees the batch; a refused install frees the result
    TextUpdate u;
    u.new_texts = {"zz"};
    fail_entry = "merge";
    calls.clear();
    bool thrown = false;
    try {
      (void)update_text_resident(ix, cur, u);
    } catch (const Error&) {
      thrown = true;
    }
    CHECK(thrown && (calls == Names{"text_sizes", "build", "fallback", "sizes(batch)", "merge", "free(batch)", "free(null)"}));
    fail_entry = "install";
    calls.clear();
    thrown = false;
    try {
      (void)update_text_resident(ix, cur, u);
    } catch (const Error&) {
      thrown = true;
    }
    CHECK(thrown && calls.back() == "free(result)" && calls[calls.size() - 2] == "install");
    fail_entry.clear();
  }
  {   // the batch's fallback documents: refused without a tokenize, added once with one
    TextUpdate u;
    u.new_texts = {"\xc3\xbc" "ber"};
    fallback = {0};
    calls.clear();
    bool thrown = false;
    try {
      (void)update_text_resident(ix, cur, u);
    } catch (const Error& e) {
      thrown = std::string(e.what()).find("batch document 0 is not reproduced") != std::string::npos;
    }
    CHECK(thrown && std::find(calls.begin(), calls.end(), "merge") == calls.end());
    calls.clear();
    const ResidentTextIndex r = update_text_resident(ix, cur, u, [] {}, Tokenizer::Unicode61, [&](const V& ids) {
      CHECK((ids == V{0}));
      TextInstances t;
      t.terms = {"uber"};
      t.inst_term = {0};
      t.inst_doc = {0};
      t.inst_pos = {0};
      return t;
    });
    CHECK((calls == plus(plus({"text_sizes", "build", "fallback", "add", "sizes(batch)", "merge", "free(batch)"}, install), {"free(result)"})));
    CHECK((r.fallback_docs == V{0}));
    fallback.clear();
  }
  {   // refused before the library is touched beyond the sizes: rows outside the table, a vocabulary of another length
    TextUpdate u;
    u.delete_ids = {5};
    calls.clear();
    bool thrown = false;
    try {
      (void)update_text_resident(ix, cur, u);
    } catch (const Error& e) {
      thrown = std::string(e.what()).find("row 5 is outside the table's 5 row ids") != std::string::npos;
    }
    CHECK(thrown && (calls == Names{"text_sizes", "free(null)"}));   // (the empty result handle goes out of scope)
    held_terms = 3;
    calls.clear();
    thrown = false;
    try {
      (void)update_text_resident(ix, cur, TextUpdate{});
    } catch (const Error& e) {
      thrown = std::string(e.what()).find("base_term_byte_offsets describes 2 terms, the handle's keyword index holds 3") != std::string::npos;
    }
    CHECK(thrown && (calls == Names{"text_sizes", "free(null)"}));
    held_terms = 2;
  }
  {   // the read-back: arrays sized from np_hip_index_text_sizes
    calls.clear();
    const BuiltTextIndex b = get_text(ix, cur.terms);
    CHECK((calls == Names{"text_sizes", "get_text"}) && (b.term_offsets == V{0, 2, 4}) && (b.inst_doc == V{0, 1, 2, 3}) && b.n_rows == 5);
    CHECK((b.inst_pos == std::vector<int32_t>{10, 11, 12, 13}));
    calls.clear();
    const TextLayout l = get_text_layout(ix);
    CHECK((calls == Names{"text_sizes", "get_text_layout"}) && (l.post_off == V{0, 1, 2}) && l.post_doc.size() == 3 && l.doc_len.size() == 5);
    bool thrown = false;
    try {
      (void)get_text(ix, {"ab"});
    } catch (const Error&) {
      thrown = true;
    }
    CHECK(thrown);
  }
  if (!failed) std::printf("all checks passed\n");
  return failed ? 1 : 0;
}
