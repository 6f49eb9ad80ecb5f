// Runs the host logic of np_textres_plan.h stand-alone (no device, no library): the byte plans of
// np_hip_index_set_text_build and np_hip_index_text_merge against sums written out here, every refusal with its message,
// the check's rule and the offender's message.  Prints "all checks passed".
#include <iostream>
#include <string>
#include "../../next-plaid_amd/csrc/np_textres_plan.h"

using namespace np;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::cout << "FAILED line " << __LINE__ << ": " #cond << "\n";       \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

static int64_t up(int64_t v) { return (v + 255) / 256 * 256; }

// the install's arrays, one by one
static int64_t install_sum(int64_t T, int64_t n, int64_t docs) {
  const int64_t m = (n > docs ? n : docs) + 1;
  int64_t t = 0;
  t += up((T + 1) * 8);             // term_offsets
  t += up((n + 1) * 8);             // inst_doc
  t += up((n + 1) * 4);             // inst_pos, the handle's pos afterwards
  t += up(m * 4);                   // flags
  t += up(m * 4);                   // their scan
  t += up(((m + 2047) / 2048 + 1) * 8);   // the scan's block sums
  t += up(((n + 2047) / 2048 + 1) * 8);   // the lowest offender per block
  t += up((T + 1) * 8);             // post_off
  t += up((n + 1) * 4);             // post_doc
  t += up((n + 1) * 4);             // post_tf
  t += up((n + 1) * 8);             // post_first
  t += up((docs > 1 ? docs : 1) * 4);   // doc_len
  return t;
}

struct Vocab {
  std::vector<uint8_t> bytes;
  std::vector<int64_t> tbo{0};
  void term(const std::string& s) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    tbo.push_back((int64_t)bytes.size());
  }
  int64_t n() const { return (int64_t)tbo.size() - 1; }
};

struct Merge {
  TextResBase base;
  Vocab a, b;
  std::vector<int64_t> remap, ids, doc_b;
  int64_t m = 0, n_rows_out = 0, limit = 0;
  bool upload = false, need = false;
  TextMergePlan plan;
  std::string why;
  int run() {
    char w[320] = "";
    TextMergeDelta d;
    d.term_bytes = b.bytes.data();
    d.term_byte_offsets = b.tbo.data();
    d.n_terms = b.n();
    d.n_inst = (int64_t)doc_b.size();
    d.n_docs = m;
    d.inst_doc = doc_b.data();
    const int rc = textres_merge_plan(base, a.bytes.data(), a.tbo.data(), remap.data(), (int64_t)remap.size(), d, ids.data(), n_rows_out,
                                      upload, limit, &plan, &need, w, sizeof(w));
    why = w;
    return rc;
  }
  bool refused(int code, const char* part) {
    const int rc = run();
    const bool ok = rc == code && why.find(part) != std::string::npos;
    if (!ok) std::cout << "  got rc " << rc << " '" << why << "'\n";
    return ok;
  }
};

static Merge sample() {
  Merge c;
  c.a.term("a");
  c.a.term("m");
  c.a.term("z");
  c.base.present = true;
  c.base.n_terms = 3;
  c.base.n_inst = 5000;
  c.base.n_docs = 6;
  c.remap = {0, -1, 1, 2, -1, 3};
  c.b.term("b");
  c.b.term("m");
  c.doc_b = {0, 0, 1};
  c.m = 2;
  c.ids = {4, 5};
  c.n_rows_out = 6;
  return c;
}

int main() {
  // ---- the install's byte plan
  for (int64_t T : {0, 1, 7, 300}) {
    const int64_t ns[] = {0, 1, 2047, 2048, 2049, 524288, 524289, 30000000};
    for (int64_t n : ns)
      for (int64_t docs : {0, 1, 5, 300000}) CHECK(textres_install_bytes(T, n, docs) == install_sum(T, n, docs));
  }
  CHECK(textres_blocks(0) == 0 && textres_blocks(1) == 1 && textres_blocks(2048) == 1 && textres_blocks(2049) == 2);
  // ---- the install's refusals, each naming its argument
  {
    char w[320];
    TextResInstall a;
    a.finalised = true;
    CHECK(textres_check_install(a, w, sizeof(w)) == NP_OK);
    auto bad = [&](TextResInstall x, int code, const char* part) {
      const int rc = textres_check_install(x, w, sizeof(w));
      const bool ok = rc == code && std::string(w).find(part) != std::string::npos;
      if (!ok) std::cout << "  got rc " << rc << " '" << w << "'\n";
      return ok;
    };
    TextResInstall x = a;
    x.index_null = true;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "index is NULL"));
    x = a;
    x.build_null = true;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "build is NULL"));
    x = a;
    x.finalised = false;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "build is not finalised"));
    x = a;
    x.consumed = true;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "build is consumed"));
    x = a;
    x.build_device = 1;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "build was built on device 1, the index lies on device 0"));
    x = a;
    x.shard_count = 2;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "index is a shard (opened with shard_count = 2)"));
    x = a;
    x.n_inst = NP_TB_MAX_INSTANCES + 1;
    CHECK(bad(x, NP_ERR_SHAPE, "Shape error: build holds 2147483648 instances"));
    x = a;
    x.n_rows = -1;
    CHECK(bad(x, NP_ERR_INVALID_ARGUMENT, "a negative count"));
  }
  // ---- the check's rule, in np_hip_index_set_text's order, and the message
  CHECK(textres_rule(0, 0, true, 0, 0, 1) == 0);
  CHECK(textres_rule(1, 0, true, 0, 0, 1) == NP_TR_RULE_DOC && textres_rule(-1, 0, true, 0, 0, 1) == NP_TR_RULE_DOC);
  CHECK(textres_rule(5, -1, true, 0, 0, 1) == NP_TR_RULE_DOC);                 // the document's rule comes first
  CHECK(textres_rule(0, -1, true, 0, 0, 1) == NP_TR_RULE_POS);
  CHECK(textres_rule(1, 0, false, 2, 0, 3) == NP_TR_RULE_ORDER);               // the document descends
  CHECK(textres_rule(1, 4, false, 1, 4, 3) == NP_TR_RULE_ORDER);               // the position repeats
  CHECK(textres_rule(1, 4, false, 1, 3, 3) == 0 && textres_rule(2, 0, false, 1, 9, 3) == 0);
  CHECK(textres_rule(1, 0, true, 2, 0, 3) == 0);                               // a term's first instance has no predecessor
  {
    char w[240];
    textres_offender_message(NP_TR_RULE_DOC, 7, 2, 12, 0, w, sizeof(w));
    CHECK(std::string(w) == "build: instance 7: document 12 is outside the index");
    textres_offender_message(NP_TR_RULE_POS, 7, 2, 1, -3, w, sizeof(w));
    CHECK(std::string(w) == "build: instance 7: position -3 is negative");
    textres_offender_message(NP_TR_RULE_ORDER, 7, 2, 1, 3, w, sizeof(w));
    CHECK(std::string(w) == "build: instance 7 of term 2 is not after its predecessor in (document, position) order");
  }
  // ---- the merge: plan, bytes and refusals
  {
    Merge c = sample();
    CHECK(c.run() == NP_OK);
    CHECK(c.plan.n_a == 5000 && c.plan.n_a_terms == 3 && c.plan.n_b_terms == 2 && c.plan.n_union == 4 && c.plan.n_survivors == 4);
    CHECK((c.plan.ua == std::vector<uint32_t>{0, 2, 3}) && (c.plan.ub == std::vector<uint32_t>{1, 2}));
    CHECK((c.plan.bound == std::vector<int64_t>{6, 6}));
    CHECK(!c.need);
    // the host merge's bytes without pos_A, plus the flags over the handle's documents, their scan and its block sums
    const int64_t want = textmerge_bytes(3, 5000, 6, 2, 3, 2, 4, false) - up(5000 * 4 + 4) + 2 * up(7 * 4) + up(2 * 8);
    CHECK(c.plan.workspace_bytes == want);
    CHECK(c.plan.workspace_bytes == textres_merge_bytes(3, 5000, 6, 2, 3, 2, 4, false, 6));
    c.upload = true;
    CHECK(c.run() == NP_OK && c.plan.workspace_bytes == want + up(3 * 8) + up(3 * 8 + 8) + up(3 * 4 + 4));
    c.upload = false;
    c.limit = want;
    CHECK(c.run() == NP_OK);
    c.limit = want - 1;
    CHECK(c.refused(NP_ERR_OUT_OF_MEMORY, ("it needs " + std::to_string(want)).c_str()));
    c.limit = -1;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "workspace_bytes -1 is negative"));
    c = sample();
    c.n_rows_out = 5;                                 // below survivors plus batch: the device counts the survivors' documents
    CHECK(c.run() == NP_OK && c.need);
    c.n_rows_out = 1;                                 // below the batch's own documents: known here
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "n_rows_out 1 is below the 2 documents"));
    c = sample();
    c.base.index_null = true;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "index is NULL"));
    c = sample();
    c.base.present = false;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "index has no keyword index"));
    c = sample();
    c.base.shard_count = 4;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "index is a shard (opened with shard_count = 4)"));
    c = sample();
    c.base.n_inst = NP_TB_MAX_INSTANCES - 1;
    CHECK(c.refused(NP_ERR_SHAPE, "the result may hold 2147483649 instances"));
    c = sample();
    c.remap[3] = 1;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "remap[3] is 1 after 1"));
    c = sample();
    c.ids = {3, 5};
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "delta_ids[0] is 3, the id that remap[5] keeps"));
    c = sample();
    c.a.tbo[2] = c.a.tbo[1];
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "base_term_byte_offsets: term 1 is empty"));
    c = sample();
    c.a.bytes[1] = 'a';                               // "a", "a": the base's vocabulary out of order
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "base_term_bytes: terms out of order"));
    c = sample();
    c.doc_b[2] = 2;
    CHECK(c.refused(NP_ERR_INVALID_ARGUMENT, "delta: instance 2 names document 2 of 2"));
    // a handle whose index holds no term, and a remap shorter than the handle's documents (checked on the device)
    Merge e;
    e.base.present = true;
    e.base.n_docs = 3;
    e.n_rows_out = 0;
    CHECK(e.run() == NP_OK && e.plan.n_union == 0 && e.plan.n_a == 0);
  }
  if (g_failed == 0) std::cout << "all checks passed\n";
  return g_failed ? 1 : 0;
}
