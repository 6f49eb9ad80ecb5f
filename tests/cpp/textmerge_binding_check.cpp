// What next_plaid.hpp's update_text_index hands the library for each of the crate's four operations, and the refusals that
// happen before the library is touched -- with the host compiler alone.  The np_hip_text_build* entries are recording stubs
// in this translation unit (no library is linked).  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

struct stub {
  int dummy;
};
stub the_batch, the_result;
std::vector<std::string> calls;
std::vector<int64_t> fallback;
std::string got_bytes, got_base_terms;
std::vector<int64_t> got_offsets, got_remap, got_ids, got_base_off, got_base_doc, got_base_tbo;
std::vector<int32_t> got_base_pos;
int64_t got_rows_out = -1, got_base_rows = -1;
const np_text_build* got_delta = nullptr;
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

int np_hip_text_build(int32_t device, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const np_text_build_opts*,
                      np_text_build** out_build, np_text_build_report* report) {
  got_device = device;
  got_offsets.assign(offsets, offsets + n_docs + 1);
  got_bytes.assign((const char*)bytes, (size_t)offsets[n_docs]);
  *out_build = (np_text_build*)&the_batch;
  *report = np_text_build_report{};
  report->n_docs = n_docs;
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
  if (b == (np_text_build*)&the_batch) {
    CHECK(!n_terms && !term_bytes && !n_inst && !rows);
    return note("sizes(batch)");
  }
  CHECK(b == (np_text_build*)&the_result);
  *n_terms = 1, *term_bytes = 2, *n_inst = 2, *rows = got_rows_out;
  return note("sizes");
}

int np_hip_text_build_fetch(const np_text_build* b, uint8_t* tb, int64_t* tbo, int64_t* toff, int64_t* idoc, int32_t* ipos) {
  CHECK(b == (np_text_build*)&the_result);
  memcpy(tb, "zz", 2);
  tbo[0] = 0, tbo[1] = 2;
  toff[0] = 0, toff[1] = 2;
  idoc[0] = 0, idoc[1] = 1, ipos[0] = 0, ipos[1] = 0;
  return note("fetch");
}

int np_hip_text_build_merge(int32_t device, const np_text_index* base, const uint8_t* tb, const int64_t* tbo, const int64_t* remap,
                            int64_t n_remap, const np_text_build* delta, const int64_t* delta_ids, int64_t n_rows_out,
                            const np_text_merge_opts* opts, np_text_build** out_build, np_text_merge_report* report) {
  got_device = device;
  got_base_tbo.assign(tbo, tbo + base->n_terms + 1);
  got_base_terms.assign((const char*)tb, (size_t)tbo[base->n_terms]);
  got_base_off.assign(base->term_offsets, base->term_offsets + base->n_terms + 1);
  const int64_t n = base->term_offsets[base->n_terms];
  got_base_doc.assign(base->inst_doc, base->inst_doc + n);
  got_base_pos.assign(base->inst_pos, base->inst_pos + n);
  got_base_rows = base->n_rows;
  got_remap.assign(remap, remap + n_remap);
  got_delta = delta;
  const int64_t m = delta ? (int64_t)got_offsets.size() - 1 : 0;
  got_ids.assign(delta_ids, delta_ids + m);
  got_rows_out = n_rows_out;
  CHECK(opts && opts->workspace_bytes == 0 && report);
  *report = np_text_merge_report{};
  report->n_instances = 2;
  const int rc = note("merge");
  if (rc == NP_OK) *out_build = (np_text_build*)&the_result;
  return rc;
}

void np_hip_text_build_free(np_text_build* b) {
  calls.push_back(!b ? "free(null)" : b == (np_text_build*)&the_batch ? "free(batch)" : "free(result)");
}
}

using namespace next_plaid;
using Names = std::vector<std::string>;
using V = std::vector<int64_t>;

static bool refused(const BuiltTextIndex& base, const TextUpdate& u, const char* part) {
  calls.clear();
  try {
    (void)update_text_index(base, u);
  } catch (const Error& e) {
    return e.kind == Error::Config && std::string(e.what()).find(part) != std::string::npos && calls.empty();
  }
  return false;
}

int main() {
  BuiltTextIndex base;   // rows 0..4: "ab", "cd", "", "ab cd", "cd"
  base.terms = {"ab", "cd"};
  base.term_offsets = {0, 2, 5};
  base.inst_doc = {0, 3, 1, 3, 4};
  base.inst_pos = {0, 0, 0, 1, 0};
  base.n_rows = 5;
  const Names with_batch = {"build", "fallback", "sizes(batch)", "merge", "sizes", "fetch", "free(result)", "free(batch)"};
  const Names without = {"merge", "sizes", "fetch", "free(result)", "free(null)"};
  {   // index (append): every row stays, the new rows follow
    TextUpdate u;
    u.new_texts = {"zz", "", "zz ab"};
    calls.clear();
    const UpdatedTextIndex r = update_text_index(base, u, Tokenizer::Unicode61, 3);
    CHECK(calls == with_batch && got_device == 3 && got_delta == (np_text_build*)&the_batch);
    CHECK(got_bytes == "zzzz ab" && (got_offsets == V{0, 2, 2, 7}));
    CHECK((got_remap == V{0, 1, 2, 3, 4}) && (got_ids == V{5, 6, 7}) && got_rows_out == 8);
    CHECK(got_base_terms == "abcd" && (got_base_tbo == V{0, 2, 4}) && got_base_off == base.term_offsets && got_base_doc == base.inst_doc &&
          got_base_pos == base.inst_pos && got_base_rows == 5);
    CHECK((r.terms == Names{"zz"}) && (r.term_offsets == V{0, 2}) && (r.inst_doc == V{0, 1}) && r.n_rows == 8 && r.merge_report.n_instances == 2);
  }
  {   // delete alone: ids keep their holes; no batch is built
    TextUpdate u;
    u.delete_ids = {3, 1, 3};
    u.renumber = false;
    calls.clear();
    update_text_index(base, u);
    CHECK(calls == without && got_delta == nullptr && (got_remap == V{0, -1, 2, -1, 4}) && got_ids.empty() && got_rows_out == 3);
  }
  {   // delete + rebuild: the survivors numbered densely in order
    TextUpdate u;
    u.delete_ids = {1, 3};
    calls.clear();
    update_text_index(base, u);
    CHECK(calls == without && (got_remap == V{0, -1, 1, -1, 2}) && got_rows_out == 3);
  }
  {   // update_rows: the replaced rows leave the base and come back in the batch at the same ids, in id order
    TextUpdate u;
    u.replace = {{4, "four"}, {0, "zero"}};
    u.renumber = false;
    calls.clear();
    update_text_index(base, u);
    CHECK(calls == with_batch && got_bytes == "zerofour" && (got_remap == V{-1, 1, 2, 3, -1}) && (got_ids == V{0, 4}) && got_rows_out == 5);
  }
  {   // all at once, renumbered: row 1 goes, row 3 is replaced (its new id is 2), one row is appended behind the four that stay
    TextUpdate u;
    u.delete_ids = {1};
    u.replace = {{3, "three"}};
    u.new_texts = {"tail"};
    calls.clear();
    update_text_index(base, u);
    CHECK(calls == with_batch && got_bytes == "threetail" && (got_remap == V{0, -1, 1, -1, 3}) && (got_ids == V{2, 4}) && got_rows_out == 5);
  }
  {   // fallback documents of the batch: refused without a tokenizer, added once with one
    TextUpdate u;
    u.new_texts = {"caf\xc3\xa9"};
    fallback = {0};
    calls.clear();
    try {
      update_text_index(base, u);
      CHECK(!"no throw");
    } catch (const Error& e) {
      CHECK(e.kind == Error::Config && std::string(e.what()).find("batch document 0 is not reproduced") != std::string::npos);
    }
    CHECK((calls == Names{"build", "fallback", "free(null)", "free(batch)"}));
    calls.clear();
    int asked = 0;
    update_text_index(base, u, Tokenizer::Unicode61, [&](const std::vector<int64_t>& ids) {
      ++asked;
      CHECK(ids == V{0});
      TextInstances t;
      t.terms = {"caf\xc3\xa9"};
      t.inst_term = {0};
      t.inst_doc = {0};
      t.inst_pos = {0};
      return t;
    });
    CHECK(asked == 1 && (calls == Names{"build", "fallback", "add", "sizes(batch)", "merge", "sizes", "fetch", "free(result)", "free(batch)"}));
    fallback.clear();
  }
  {   // refused before the library is touched
    TextUpdate u;
    u.delete_ids = {5};
    CHECK(refused(base, u, "row 5 is outside the table's 5 row ids"));
    u.delete_ids = {-1};
    CHECK(refused(base, u, "row -1 is outside"));
    u.delete_ids = {2};
    u.replace = {{2, "x"}};
    CHECK(refused(base, u, "row 2 is in both delete and replace"));
    u.delete_ids.clear();
    u.replace = {{2, "x"}, {2, "y"}};
    CHECK(refused(base, u, "row 2 is replaced twice"));
    u.replace = {{7, "x"}};
    CHECK(refused(base, u, "row 7 is outside"));
    BuiltTextIndex odd = base;
    odd.term_offsets.pop_back();
    CHECK(refused(odd, TextUpdate(), "one entry per term and one more"));
  }
  {   // the library's refusal: the mapped kind and its message; both builds are released
    TextUpdate u;
    u.new_texts = {"zz"};
    fail_entry = "merge";
    calls.clear();
    try {
      update_text_index(base, u);
      CHECK(!"no throw");
    } catch (const Error& e) {
      CHECK(e.kind == Error::Config && std::string(e.what()) == "Invalid argument: the stub said so");
    }
    CHECK((calls == Names{"build", "fallback", "sizes(batch)", "merge", "free(null)", "free(batch)"}));
    fail_entry.clear();
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
