// Stand-alone check of text_check_expr (next-plaid_amd/csrc/np_text_plan.h): the host check of a tree query -- its phrases,
// prefix ranges and postfix node list -- that np_hip_text_search_expr runs before any launch.  No device, no library: build
// with the host compiler -- tests/test_text_expr_restate_cpu.py builds it plain and with -fsanitize=address,undefined -- and run.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "np_text_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static std::string last;
static const int BAD = NP_ERR_INVALID_ARGUMENT;
static const int P = NP_TEXT_NODE_PHRASE, AND = NP_TEXT_NODE_AND, OR = NP_TEXT_NODE_OR, NOT = NP_TEXT_NODE_NOT;

// a query from exactly-sized copies: a read past an array is a sanitizer report
struct E {
  std::vector<int32_t> terms, off, hi;
  std::vector<np_text_node> nodes;
  int check(int64_t n_terms) const {
    std::vector<int32_t> t(terms), o(off), h(hi);
    std::vector<np_text_node> n(nodes);
    np_text_expr e{t.empty() ? nullptr : t.data(), o.empty() ? nullptr : o.data(), h.empty() ? nullptr : h.data(),
                   n.empty() ? nullptr : n.data(), (int32_t)o.size() - 1, (int32_t)n.size()};
    char why[320] = "";
    const int rc = text_check_expr(&e, 3, n_terms, why, sizeof why);
    last = why;
    return rc;
  }
};

static bool says(const char* what) { return last.find(what) != std::string::npos; }

// (t0 OR "t1 t2") NOT t3*   over three phrases; the prefix stands for the terms [3, 6)
static E good() {
  E e;
  e.terms = {0, 1, 2, 3};
  e.off = {0, 1, 3, 4};
  e.hi = {0, 0, 6};
  e.nodes = {{P, 0, 0}, {P, 1, 0}, {OR, 0, 1}, {P, 2, 0}, {NOT, 2, 3}};
  return e;
}

// n leaves chained from the left (left = true) or from the right by `op`
static E chain(int n, int op, bool left) {
  E e;
  for (int i = 0; i < n; ++i) {
    e.terms.push_back(i % 5);
    e.off.push_back(i);
    e.hi.push_back(0);
  }
  e.off.push_back(n);
  if (left) {
    e.nodes.push_back({P, 0, 0});
    for (int i = 1; i < n; ++i) {
      e.nodes.push_back({P, i, 0});
      const int32_t at = (int32_t)e.nodes.size();
      e.nodes.push_back({op, i == 1 ? 0 : at - 2, at - 1});
    }
  } else {
    for (int i = 0; i < n; ++i) e.nodes.push_back({P, i, 0});
    for (int i = n - 2; i >= 0; --i) e.nodes.push_back({op, i, (int32_t)e.nodes.size() - 1});
  }
  return e;
}

int main() {
  EXPECT(good().check(10) == 0);
  EXPECT(chain(1, AND, true).check(5) == 0);
  for (int op : {AND, OR, NOT})
    for (bool left : {true, false}) {
      EXPECT(chain(64, op, left).check(5) == 0);      // 64 phrases, 127 nodes, 63 operators deep
      EXPECT(chain(2, op, left).check(5) == 0);
    }
  EXPECT(chain(65, OR, true).check(5) == BAD && says("text query 3: n_phrases = 65 must be in 1..64"));

  E e = good();   // stack underflow: an operator with one node on the stack
  e.nodes = {{P, 0, 0}, {OR, 0, 0}, {P, 1, 0}, {P, 2, 0}, {NOT, 2, 3}};
  EXPECT(e.check(10) == BAD && says("node 1: the stack holds 1 nodes, an operator needs two"));
  e = good();     // ... with none
  e.nodes = {{AND, 0, 0}, {P, 0, 0}, {P, 1, 0}, {P, 2, 0}, {OR, 2, 3}};
  EXPECT(e.check(10) == BAD && says("node 0: the stack holds 0 nodes"));
  e = good();     // a dangling node: two are left at the end
  e.nodes = {{P, 0, 0}, {P, 1, 0}, {OR, 0, 1}, {P, 2, 0}};
  EXPECT(e.check(10) == BAD && says("2 nodes are left on the stack at the end, not one"));
  e = good();     // a phrase used twice (and one never)
  e.nodes[3] = {P, 1, 0};
  EXPECT(e.check(10) == BAD && says("node 3 names phrase 1 a second time"));
  e = good();
  e.nodes = {{P, 0, 0}, {P, 1, 0}, {OR, 0, 1}};
  EXPECT(e.check(10) == BAD && says("phrase 2 is named by no node"));
  e = good();
  e.nodes[3] = {P, 3, 0};
  EXPECT(e.check(10) == BAD && says("node 3 names phrase 3, which the query does not have"));
  e = good();
  e.nodes[3] = {P, -1, 0};
  EXPECT(e.check(10) == BAD && says("names phrase -1"));
  e = good();     // children: not below the parent, not the top of the stack, swapped
  e.nodes[4] = {NOT, 2, 4};
  EXPECT(e.check(10) == BAD && says("node 4: a child index is not below the node's own"));
  e.nodes[4] = {NOT, 2, 5};
  EXPECT(e.check(10) == BAD && says("node 4: a child index"));
  e.nodes[4] = {NOT, -1, 3};
  EXPECT(e.check(10) == BAD && says("node 4: a child index"));
  e.nodes[4] = {NOT, 0, 3};
  EXPECT(e.check(10) == BAD && says("node 4: its children are not the two nodes on top of the stack"));
  e.nodes[4] = {NOT, 3, 2};
  EXPECT(e.check(10) == BAD && says("node 4: its children are not the two nodes on top of the stack"));
  e.nodes[4] = {9, 2, 3};
  EXPECT(e.check(10) == BAD && says("node 4: unknown op 9"));
  e = good();
  e.nodes.clear();
  EXPECT(e.check(10) == BAD && says("n_nodes = 0 must be in 1..127"));
  e = chain(64, OR, true);
  e.nodes.push_back({P, 0, 0});
  EXPECT(e.check(5) == BAD && says("n_nodes = 128"));

  // prefix ranges: inside the vocabulary, after the phrase's last term, which is their start
  e = good();
  EXPECT(e.check(6) == 0);
  EXPECT(e.check(5) == BAD && says("phrase 2: the prefix range ends at 6, outside the vocabulary"));
  e.hi[2] = 3;
  EXPECT(e.check(10) == BAD && says("phrase 2: the prefix range ends at 3"));
  e.hi[2] = -2;
  EXPECT(e.check(10) == BAD && says("phrase 2: the prefix range ends at -2"));
  e = good();
  e.terms[3] = -1;
  EXPECT(e.check(10) == BAD && says("phrase 2: a prefix range needs a known last token"));
  e = good();     // the cap of a phrase of several tokens; a single-token phrase has none
  e.hi = {0, 2 + NP_TEXT_MAX_PREFIX_TERMS, 3 + 5000};
  EXPECT(e.check(10000) == 0);
  e.hi[1] = 2 + NP_TEXT_MAX_PREFIX_TERMS + 1;
  EXPECT(e.check(10000) == BAD && says("phrase 1 of several tokens ends in a prefix of 1025 terms, more than NP_TEXT_MAX_PREFIX_TERMS = 1024"));

  // the phrases, as text_check_query checks them
  e = good();
  e.off = {0, 1, 1, 4};
  EXPECT(e.check(10) == BAD && says("phrase 1 has no token"));
  e = good();
  e.off[0] = 1;
  EXPECT(e.check(10) == BAD && says("phrase_offsets[0] = 1 must be 0"));
  e = good();
  e.terms[1] = 10;
  EXPECT(e.check(10) == BAD && says("token 1 names no term of the vocabulary"));
  e.terms[1] = -2;
  EXPECT(e.check(10) == BAD && says("token 1 names no term"));
  e.terms[1] = -1;
  EXPECT(e.check(10) == 0);
  e = good();
  e.terms.assign(257, 1);
  e.off = {0, 1, 256, 257};
  e.hi = {0, 0, 0};
  EXPECT(e.check(10) == BAD && says("more than 256 tokens (at phrase 2)"));
  e.terms.assign(256, 1);
  e.off = {0, 1, 255, 256};
  EXPECT(e.check(10) == 0);
  e = good();
  e.hi.clear();
  EXPECT(e.check(10) == BAD && says("NULL phrase_offsets, terms, prefix_hi or nodes"));
  char why[320] = "";
  EXPECT(text_check_expr(nullptr, 0, 1, why, sizeof why) == BAD && std::strstr(why, "NULL query"));

  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
