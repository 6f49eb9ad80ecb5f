// Runs the host logic of np_textmerge_plan.h stand-alone (no device, no library).
// Without input: the vocabulary union, `bound`, every refusal with its message, the string compaction and the workspace
// plan against hand-written answers; prints "all checks passed".
// With input (tests/test_textmerge_restate_cpu.py; whitespace-separated integers), per command
//   PLAN <strings A> <vec toff_A> <vec doc_A> <vec pos_A> <vec remap> <strings B> <vec toff_B> <vec doc_B> <vec delta_ids> m n_rows_out
//     strings: n {len byte*len}*n      vec: n value*n
// it prints "rc code why", "ua ...", "ub ...", "bound ...".
#include <iostream>
#include <string>
#include "../../next-plaid_amd/csrc/np_textmerge_plan.h"

using namespace np;

static int g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::cout << "FAILED line " << __LINE__ << ": " #cond << "\n";       \
      ++g_failed;                                                          \
    }                                                                      \
  } while (0)

struct Side {
  std::vector<uint8_t> bytes;
  std::vector<int64_t> tbo{0}, toff{0}, doc;
  std::vector<int32_t> pos;
  void term(const std::string& s, std::vector<std::pair<int64_t, int32_t>> inst) {
    bytes.insert(bytes.end(), s.begin(), s.end());
    tbo.push_back((int64_t)bytes.size());
    for (auto& p : inst) doc.push_back(p.first), pos.push_back(p.second);
    toff.push_back((int64_t)doc.size());
  }
  int64_t n_terms() const { return (int64_t)tbo.size() - 1; }
  np_text_index index(int64_t n_rows) const {
    np_text_index t = {};
    t.n_terms = n_terms();
    t.term_offsets = toff.data();
    t.inst_doc = doc.data();
    t.inst_pos = pos.data();
    t.n_rows = n_rows;
    return t;
  }
  TextMergeDelta delta(int64_t n_docs) const {
    TextMergeDelta d;
    d.term_bytes = bytes.data();
    d.term_byte_offsets = tbo.data();
    d.n_terms = n_terms();
    d.n_inst = (int64_t)doc.size();
    d.n_docs = n_docs;
    d.inst_doc = doc.data();
    return d;
  }
};

struct Call {
  Side a, b;
  std::vector<int64_t> remap, ids;
  int64_t a_rows = 0, m = 0, n_rows_out = 0, limit = 0;
  bool upload = false;
  TextMergePlan plan;
  std::string why;
  int run() {
    char w[256] = "";
    const np_text_index t = a.index(a_rows);
    const int rc = textmerge_plan(&t, a.bytes.data(), a.tbo.data(), remap.data(), (int64_t)remap.size(), b.delta(m), ids.data(), n_rows_out,
                                  upload, limit, &plan, w, sizeof(w));
    why = w;
    return rc;
  }
  bool refused(int code, const char* part) {
    const int rc = run();
    if (rc != code || why.find(part) == std::string::npos) {
      std::cout << "got rc " << rc << " why '" << why << "', wanted " << code << " with '" << part << "'\n";
      return false;
    }
    return true;
  }
};

// A: "a" in documents 0, 2; "ab" in 1, 2 (twice); "c" in 3.  Four old documents.
static Call good() {
  Call c;
  c.a.term("a", {{0, 0}, {2, 1}});
  c.a.term("ab", {{1, 0}, {2, 0}, {2, 2}});
  c.a.term("c", {{3, 0}});
  c.a_rows = 4;
  c.remap = {0, -1, 1, 3};   // document 1 removed; 0 -> 0, 2 -> 1, 3 -> 3
  // B: two documents at the new ids 2 and 4; "0" and "ab" in document 0, "ab" and "b" in document 1
  c.b.term("0", {{0, 0}});
  c.b.term("ab", {{0, 1}, {1, 0}});
  c.b.term("b", {{1, 1}});
  c.m = 2;
  c.ids = {2, 4};
  c.n_rows_out = 5;
  return c;
}

static void self_checks() {
  {
    Call c = good();
    CHECK(c.run() == NP_OK);
    const TextMergePlan& p = c.plan;
    // union: 0(B) a(A) ab(both) b(B) c(A)
    CHECK(p.n_union == 5 && p.n_a == 6 && p.n_b == 4 && p.n_survivors == 3);
    CHECK((p.ua == std::vector<uint32_t>{1, 2, 4}) && (p.ub == std::vector<uint32_t>{0, 2, 3}));
    CHECK((p.a_of == std::vector<int32_t>{-1, 0, 1, -1, 2}) && (p.b_of == std::vector<int32_t>{0, -1, 1, 2, -1}));
    // new id 2 lies between old 2 (-> 1) and old 3 (-> 3): bound 3; new id 4 lies above all: bound n_remap
    CHECK((p.bound == std::vector<int64_t>{3, 4}));
    CHECK(p.workspace_bytes == textmerge_bytes(3, 6, 4, 3, 4, 2, 5, false) && p.workspace_bytes % 256 == 0);
    const uint32_t alive[5] = {1, 1, 1, 0, 1};
    std::vector<uint8_t> bytes;
    std::vector<int64_t> tbo;
    textmerge_compact_terms(p, alive, c.a.bytes.data(), c.a.tbo.data(), c.b.bytes.data(), c.b.tbo.data(), &bytes, &tbo);
    CHECK(std::string(bytes.begin(), bytes.end()) == "0aabc" && (tbo == std::vector<int64_t>{0, 1, 2, 4, 5}));
  }
  {   // the shorter string first; a prefix on either side; an empty side
    Call c;
    c.a.term("ab", {{0, 0}});
    c.a.term("abc", {{0, 1}});
    c.a_rows = 1;
    c.remap = {0};
    c.b.term("a", {{0, 0}});
    c.b.term("abcd", {{0, 1}});
    c.m = 1;
    c.ids = {1};
    c.n_rows_out = 2;
    CHECK(c.run() == NP_OK);
    CHECK((c.plan.ua == std::vector<uint32_t>{1, 2}) && (c.plan.ub == std::vector<uint32_t>{0, 3}) && (c.plan.bound == std::vector<int64_t>{1}));
    Call e;
    e.n_rows_out = 0;
    CHECK(e.run() == NP_OK && e.plan.n_union == 0 && e.plan.bound.empty());
    Call only_b = c;
    only_b.a = Side();
    only_b.a_rows = 0;
    only_b.remap.clear();
    only_b.ids = {0};
    CHECK(only_b.run() == NP_OK && only_b.plan.n_union == 2 && (only_b.plan.bound == std::vector<int64_t>{0}));
  }
  {   // bound with holes in remap and ids kept (no renumbering): remap = {-1, 5, -1, 9}
    Call c;
    c.a.term("x", {{1, 0}, {3, 0}});
    c.a_rows = 2;
    c.remap = {-1, 5, -1, 9};
    c.m = 4;
    c.ids = {0, 6, 8, 10};
    c.n_rows_out = 6;
    CHECK(c.run() == NP_OK && (c.plan.bound == std::vector<int64_t>{1, 3, 3, 4}));
  }
  // ---- the refusals, each naming its argument
  const int INV = NP_ERR_INVALID_ARGUMENT;
  { Call c = good(); c.a.toff[0] = 1; CHECK(c.refused(INV, "base: term_offsets[0] = 1 must be 0")); }
  { Call c = good(); c.a.toff[2] = 1; CHECK(c.refused(INV, "base: term_offsets decrease at term 1")); }
  { Call c = good(); c.a.pos[4] = 0; CHECK(c.refused(INV, "base: instance 4 of term 1 is not after its predecessor")); }
  { Call c = good(); c.a.pos[0] = -1; CHECK(c.refused(INV, "base: instance 0: position -1 is negative")); }
  { Call c = good(); c.a_rows = 3; CHECK(c.refused(INV, "base: n_rows = 3 is below the 4 documents")); }
  { Call c = good(); c.a.doc[5] = 4; CHECK(c.refused(INV, "base: instance 5: document 4 is outside the index (the index is n_remap = 4")); }
  { Call c = good(); c.a.bytes[0] = 'b'; CHECK(c.refused(INV, "base_term_bytes: terms out of order: term 1 does not sort after term 0")); }
  { Call c = good(); c.a.tbo[1] = 0; CHECK(c.refused(INV, "base_term_byte_offsets: term 0 is empty")); }
  { Call c = good(); c.b.bytes[0] = 'z'; CHECK(c.refused(INV, "delta_term_bytes: terms out of order")); }
  { Call c = good(); c.remap = {0, -1, 0, 3}; CHECK(c.refused(INV, "remap[2] is 0 after 0: the survivors' ids must ascend strictly")); }
  { Call c = good(); c.remap = {2, -1, 1, 3}; CHECK(c.refused(INV, "remap[2] is 1 after 2")); }
  { Call c = good(); c.remap[1] = -2; CHECK(c.refused(INV, "remap[1] is -2")); }
  { Call c = good(); c.ids = {4, 2}; CHECK(c.refused(INV, "delta_ids[1] is 2 after 4: the ids must ascend strictly")); }
  { Call c = good(); c.ids = {2, 2}; CHECK(c.refused(INV, "delta_ids[1] is 2 after 2")); }
  { Call c = good(); c.ids = {1, 4}; CHECK(c.refused(INV, "delta_ids[0] is 1, the id that remap[2] keeps")); }
  { Call c = good(); c.ids = {-1, 4}; CHECK(c.refused(INV, "delta_ids[0] is -1, a negative id")); }
  { Call c = good(); c.n_rows_out = 4; CHECK(c.refused(INV, "n_rows_out 4 is below the 5 documents of the result")); }
  {   // a batch document without a token does not count: 5 rows hold the result's 5 documents with a token, 4 do not
    Call c = good();
    c.m = 3;
    c.ids = {2, 4, 5};
    CHECK(c.run() == NP_OK && (c.plan.bound == std::vector<int64_t>{3, 4, 4}));
    c.n_rows_out = 4;
    CHECK(c.refused(INV, "n_rows_out 4 is below the 5 documents of the result"));
  }
  { Call c = good(); c.n_rows_out = -1; CHECK(c.refused(INV, "n_rows_out -1 is negative")); }
  { Call c = good(); c.b.doc[3] = 2; CHECK(c.refused(INV, "delta: instance 3 names document 2 of 2")); }
  {
    Call c = good();
    const np_text_index t = c.a.index(4);
    char w[256];
    CHECK(textmerge_plan(&t, c.a.bytes.data(), c.a.tbo.data(), nullptr, 4, c.b.delta(2), c.ids.data(), 5, false, 0, &c.plan, w, sizeof(w)) == INV &&
          std::string(w) == "remap is NULL");
    CHECK(textmerge_plan(&t, c.a.bytes.data(), c.a.tbo.data(), c.remap.data(), 4, c.b.delta(2), nullptr, 5, false, 0, &c.plan, w, sizeof(w)) == INV &&
          std::string(w) == "delta_ids is NULL");
    CHECK(textmerge_plan(nullptr, nullptr, nullptr, c.remap.data(), 4, c.b.delta(2), c.ids.data(), 5, false, 0, &c.plan, w, sizeof(w)) == INV &&
          std::string(w) == "base is NULL");
    CHECK(textmerge_plan(&t, c.a.bytes.data(), c.a.tbo.data(), c.remap.data(), -1, c.b.delta(2), c.ids.data(), 5, false, 0, &c.plan, w, sizeof(w)) ==
              INV && std::string(w) == "n_remap -1 is negative");
  }
  {   // shapes: 2^31 instances on either side or in the sum (the offsets alone say so; no instance is read)
    Call c = good();
    TextMergeDelta d = c.b.delta(2);
    d.n_inst = (int64_t)1 << 31;
    const np_text_index t = c.a.index(4);
    char w[256];
    CHECK(textmerge_plan(&t, c.a.bytes.data(), c.a.tbo.data(), c.remap.data(), 4, d, c.ids.data(), 5, false, 0, &c.plan, w, sizeof(w)) == NP_ERR_SHAPE &&
          std::string(w).find("delta holds 2147483648 instances") != std::string::npos);
    const int64_t toff[2] = {0, (int64_t)1 << 31};
    np_text_index big = {};
    big.n_terms = 1, big.term_offsets = toff, big.n_rows = 1;
    CHECK(textmerge_plan(&big, c.a.bytes.data(), c.a.tbo.data(), c.remap.data(), 4, c.b.delta(2), c.ids.data(), 5, false, 0, &c.plan, w, sizeof(w)) ==
              NP_ERR_SHAPE && std::string(w).find("base holds 2147483648 instances") != std::string::npos);
  }
  {   // the workspace: the planned bytes pass, one byte less does not; an uploaded batch needs more
    Call c = good();
    CHECK(c.run() == NP_OK);
    const int64_t need = c.plan.workspace_bytes;
    c.limit = need;
    CHECK(c.run() == NP_OK);
    c.limit = need - 1;
    CHECK(c.refused(NP_ERR_OUT_OF_MEMORY, "does not hold the call"));
    c.limit = -5;
    CHECK(c.refused(INV, "workspace_bytes -5 is negative"));
    c.limit = 0;
    c.upload = true;
    CHECK(c.run() == NP_OK && c.plan.workspace_bytes == need + 3 * 256);
    CHECK(textmerge_bytes(0, 0, 0, 0, 0, 0, 0, false) == 20 * 256);
  }
}

static void read_strings(Side* s) {
  int64_t n;
  std::cin >> n;
  for (int64_t i = 0; i < n; ++i) {
    int64_t len;
    std::cin >> len;
    for (int64_t j = 0; j < len; ++j) {
      int v;
      std::cin >> v;
      s->bytes.push_back((uint8_t)v);
    }
    s->tbo.push_back((int64_t)s->bytes.size());
  }
}

template <class T>
static void read_vec(std::vector<T>* v) {
  int64_t n;
  std::cin >> n;
  v->resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    int64_t x;
    std::cin >> x;
    (*v)[(size_t)i] = (T)x;
  }
}

int main() {
  std::string cmd;
  bool any = false;
  while (std::cin >> cmd) {
    any = true;
    if (cmd != "PLAN") {
      std::cout << "unknown command " << cmd << "\n";
      return 2;
    }
    Call c;
    read_strings(&c.a);
    read_vec(&c.a.toff);
    read_vec(&c.a.doc);
    read_vec(&c.a.pos);
    read_vec(&c.remap);
    read_strings(&c.b);
    read_vec(&c.b.toff);
    read_vec(&c.b.doc);
    read_vec(&c.ids);
    std::cin >> c.m >> c.n_rows_out;
    c.a_rows = (int64_t)c.remap.size();
    const int rc = c.run();
    std::cout << "rc " << rc << " " << c.why << "\nua";
    for (uint32_t v : c.plan.ua) std::cout << " " << v;
    std::cout << "\nub";
    for (uint32_t v : c.plan.ub) std::cout << " " << v;
    std::cout << "\nbound";
    for (int64_t v : c.plan.bound) std::cout << " " << v;
    std::cout << "\n";
  }
  if (!any) {
    self_checks();
    if (g_failed) return 1;
    std::cout << "all checks passed\n";
  }
  return 0;
}
