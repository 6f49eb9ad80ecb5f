// What next_plaid.hpp's build_text_index hands the library, and what it makes of the answer -- with the host compiler alone.
// The six np_hip_text_build* entries are recording stubs in this translation unit (no library is linked): each notes its
// name and the values behind its arguments and writes a chosen answer through the output pointers.  Built with
// -fsanitize=address,undefined: an array the header sized too small is an error here.
#include <cstdio>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

struct np_text_build_stub {
  int dummy;
};
np_text_build_stub the_build;
std::vector<std::string> calls;
std::vector<int64_t> fallback;              // what the stub device hands back
std::string got_bytes;
std::vector<int64_t> got_offsets, added_doc;
std::vector<std::string> added_terms;
std::vector<int32_t> added_term, added_pos;
np_text_build_opts got_opts{};
int got_device = -1, fail_entry_rc = 0;
std::string fail_entry;
int failed = 0;
// the stub's result
const std::vector<std::string> R_TERMS = {"ab", "cd"};
const std::vector<int64_t> R_OFF = {0, 1, 3}, R_DOC = {0, 0, 2};
const std::vector<int32_t> R_POS = {0, 1, 0};
int64_t n_rows = 0;

#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

int note(const char* name) {
  calls.push_back(name);
  return fail_entry == name ? fail_entry_rc : NP_OK;
}

}  // namespace

extern "C" {
const char* np_hip_last_error(void) { return "Invalid argument: the stub said so"; }

int np_hip_text_build(int32_t device, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const np_text_build_opts* opts,
                      np_text_build** out_build, np_text_build_report* report) {
  got_device = device;
  got_offsets.assign(offsets, offsets + n_docs + 1);
  got_bytes.assign((const char*)bytes, (size_t)offsets[n_docs]);
  got_opts = *opts;
  n_rows = n_docs;
  const int rc = note("build");
  if (rc != NP_OK) return rc;
  *out_build = (np_text_build*)&the_build;
  *report = np_text_build_report{};
  report->n_docs = n_docs;
  report->n_fallback = (int64_t)fallback.size();
  report->n_instances = 3;
  return NP_OK;
}

int np_hip_text_build_fallback(const np_text_build* b, int64_t* ids, int64_t* count) {
  CHECK(b == (np_text_build*)&the_build);
  for (size_t i = 0; i < fallback.size(); ++i) ids[i] = fallback[i];
  if (count) *count = (int64_t)fallback.size();
  return note("fallback");
}

int np_hip_text_build_add(np_text_build* b, const uint8_t* tb, const int64_t* tbo, int64_t n_terms, const int32_t* it,
                          const int64_t* idoc, const int32_t* ipos, int64_t n) {
  CHECK(b == (np_text_build*)&the_build);
  added_terms.clear();
  for (int64_t t = 0; t < n_terms; ++t) added_terms.emplace_back((const char*)tb + tbo[t], (size_t)(tbo[t + 1] - tbo[t]));
  added_term.assign(it, it + n);
  added_doc.assign(idoc, idoc + n);
  added_pos.assign(ipos, ipos + n);
  return note("add");
}

int np_hip_text_build_sizes(np_text_build* b, int64_t* n_terms, int64_t* term_bytes, int64_t* n_inst, int64_t* rows) {
  CHECK(b == (np_text_build*)&the_build);
  *n_terms = (int64_t)R_TERMS.size();
  *term_bytes = 4;
  *n_inst = (int64_t)R_DOC.size();
  *rows = n_rows;
  return note("sizes");
}

int np_hip_text_build_fetch(const np_text_build* b, uint8_t* tb, int64_t* tbo, int64_t* toff, int64_t* idoc, int32_t* ipos) {
  CHECK(b == (np_text_build*)&the_build);
  memcpy(tb, "abcd", 4);
  tbo[0] = 0, tbo[1] = 2, tbo[2] = 4;
  for (size_t i = 0; i < R_OFF.size(); ++i) toff[i] = R_OFF[i];
  for (size_t i = 0; i < R_DOC.size(); ++i) idoc[i] = R_DOC[i], ipos[i] = R_POS[i];
  return note("fetch");
}

void np_hip_text_build_free(np_text_build* b) {
  if (b) CHECK(b == (np_text_build*)&the_build);
  calls.push_back(b ? "free" : "free(null)");
}
}

using namespace next_plaid;
using Names = std::vector<std::string>;

int main() {
  const std::vector<std::string> texts = {"ab cd", "", "cd"};
  {   // no fallback: build, fallback, sizes, fetch, free; the arrays as the stub wrote them
    calls.clear();
    const BuiltTextIndex r = build_text_index(texts, Tokenizer::Unicode61, 2, 99);
    CHECK((calls == Names{"build", "fallback", "sizes", "fetch", "free"}));
    CHECK(got_bytes == "ab cdcd" && (got_offsets == std::vector<int64_t>{0, 5, 5, 7}) && got_device == 2);
    CHECK(got_opts.tokenizer == NP_TOK_UNICODE61 && got_opts.max_token_bytes == 99 && got_opts.hash_bits == 0 &&
          got_opts.tile_bytes == 0 && got_opts.workspace_bytes == 0);
    CHECK(r.terms == R_TERMS && r.term_offsets == R_OFF && r.inst_doc == R_DOC && r.inst_pos == R_POS && r.n_rows == 3);
    CHECK(r.fallback_docs.empty() && r.report.n_instances == 3);
  }
  {   // a fallback list: returned to the caller; with the caller's tokenizer its instances are added once
    fallback = {1, 4};
    calls.clear();
    const BuiltTextIndex plain = build_text_index(texts, Tokenizer::Trigram);
    CHECK((calls == Names{"build", "fallback", "sizes", "fetch", "free"}));
    CHECK(got_opts.tokenizer == NP_TOK_TRIGRAM && (plain.fallback_docs == std::vector<int64_t>{1, 4}));
    calls.clear();
    int asked = 0;
    const BuiltTextIndex r = build_text_index(texts, Tokenizer::Unicode61, [&](const std::vector<int64_t>& ids) {
      ++asked;
      CHECK((ids == std::vector<int64_t>{1, 4}));
      TextInstances t;
      t.terms = {"x", "\xc3\xa9"};
      t.inst_term = {0, 1, 1};
      t.inst_doc = {1, 1, 4};
      t.inst_pos = {0, 1, 0};
      return t;
    });
    CHECK(asked == 1 && (calls == Names{"build", "fallback", "add", "sizes", "fetch", "free"}));
    CHECK((added_terms == Names{"x", "\xc3\xa9"}) && (added_term == std::vector<int32_t>{0, 1, 1}) &&
          (added_doc == std::vector<int64_t>{1, 1, 4}) && (added_pos == std::vector<int32_t>{0, 1, 0}));
    CHECK((r.fallback_docs == std::vector<int64_t>{1, 4}) && r.terms == R_TERMS);
    fallback.clear();
    calls.clear();
    asked = 0;
    build_text_index(texts, Tokenizer::Unicode61, [&](const std::vector<int64_t>&) { return ++asked, TextInstances{}; });
    CHECK(asked == 0 && (calls == Names{"build", "fallback", "sizes", "fetch", "free"}));   // nothing to tokenise: no add
  }
  {   // errors: the mapped kind and the message; the build is released whenever one came back
    calls.clear();
    fail_entry = "build", fail_entry_rc = NP_ERR_SHAPE;
    try {
      build_text_index(texts);
      CHECK(!"no throw");
    } catch (const Error& e) {
      CHECK(e.kind == Error::Shape && std::string(e.what()) == "Invalid argument: the stub said so");
    }
    CHECK((calls == Names{"build", "free(null)"}));
    calls.clear();
    fallback = {0};
    fail_entry = "add", fail_entry_rc = NP_ERR_INVALID_ARGUMENT;
    try {
      build_text_index(texts, Tokenizer::Unicode61, [&](const std::vector<int64_t>&) { return TextInstances{}; });
      CHECK(!"no throw");
    } catch (const Error& e) {
      CHECK(e.kind == Error::Config);
    }
    CHECK((calls == Names{"build", "fallback", "add", "free"}));
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
