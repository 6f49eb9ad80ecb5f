// Stand-alone check of the host code behind the counting exchange of a sharded tree batch (next-plaid_amd/csrc/np_text_plan.h:
// text_counted_expr_phrases, which sizes the count vector from the queries alone, and text_prefix_bitmap_bytes /
// text_prefix_group, which cut the counting pre-pass into groups of bitmaps).  No device, no library: build with the host
// compiler -- tests/test_shard_text_expr_restate_cpu.py builds it plain and with -fsanitize=address,undefined -- and run.
// The queries live in exactly-sized heap arrays: a read one past the end is a report.
#include <cstdio>
#include <memory>
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

// a tree query over exactly-sized heap arrays: the phrases chained by ANDs
struct Expr {
  std::unique_ptr<int32_t[]> terms, off, hi;
  std::unique_ptr<np_text_node[]> nodes;
  np_text_expr e{};
  Expr(const std::vector<std::vector<int32_t>>& phrases, const std::vector<int32_t>& prefix_hi) {
    const int n = (int)phrases.size();
    size_t nt = 0;
    for (const auto& p : phrases) nt += p.size();
    terms.reset(new int32_t[nt]);
    off.reset(new int32_t[n + 1]);
    hi.reset(new int32_t[n]);
    nodes.reset(new np_text_node[2 * n - 1]);
    size_t k = 0;
    int nn = 0;
    off[0] = 0;
    for (int p = 0; p < n; ++p) {
      for (int32_t t : phrases[p]) terms[k++] = t;
      off[p + 1] = (int32_t)k;
      hi[p] = prefix_hi[p];
      nodes[nn++] = np_text_node{NP_TEXT_NODE_PHRASE, p, 0};
      if (p > 0) {
        nodes[nn] = np_text_node{NP_TEXT_NODE_AND, p == 1 ? 0 : nn - 2, nn - 1};
        ++nn;
      }
    }
    e = np_text_expr{terms.get(), off.get(), hi.get(), nodes.get(), n, nn};
  }
};

static void counted_phrases() {
  // exact single | single prefix | several tokens | several ending in a prefix | unknown single | unknown in several (prefix)
  Expr a({{3}, {5}, {1, 2}, {4, 6}, {-1}, {-1, 7}}, {0, 9, 0, 8, 0, 9});
  // one prefix phrase alone; a query without any counted phrase
  Expr b({{0}}, {12});
  Expr c({{2}, {-1}}, {0, 0});
  char why[320];
  for (const Expr* x : {&a, &b, &c}) EXPECT(text_check_expr(&x->e, 0, 16, why, sizeof why) == 0);
  std::unique_ptr<np_text_expr[]> batch(new np_text_expr[3]{a.e, b.e, c.e});
  int64_t multi = -1, prefix = -1;
  EXPECT(text_counted_expr_phrases(batch.get(), 3, &multi, &prefix) == 4 && multi == 2 && prefix == 2);
  EXPECT(text_counted_expr_phrases(batch.get(), 1) == 3);
  EXPECT(text_counted_expr_phrases(batch.get() + 1, 1, &multi, &prefix) == 1 && multi == 0 && prefix == 1);
  EXPECT(text_counted_expr_phrases(batch.get() + 2, 1, &multi, &prefix) == 0 && multi == 0 && prefix == 0);
  EXPECT(text_counted_expr_phrases(batch.get(), 0) == 0 && text_counted_expr_phrases(nullptr, 0, &multi, nullptr) == 0 && multi == 0);
  // the limits of one query: 64 single-token prefix phrases (127 nodes), and 64 phrases over 256 tokens
  std::vector<std::vector<int32_t>> many(NP_TEXT_MAX_PHRASES, std::vector<int32_t>{1});
  Expr d(many, std::vector<int32_t>(NP_TEXT_MAX_PHRASES, 5));
  EXPECT(d.e.n_nodes == NP_TEXT_MAX_NODES && text_check_expr(&d.e, 0, 16, why, sizeof why) == 0);
  EXPECT(text_counted_expr_phrases(&d.e, 1, &multi, &prefix) == 64 && prefix == 64);
  std::vector<std::vector<int32_t>> wide(NP_TEXT_MAX_PHRASES, std::vector<int32_t>{1, 2, 3, 4});
  Expr w(wide, std::vector<int32_t>(NP_TEXT_MAX_PHRASES, 0));
  EXPECT(w.e.phrase_offsets[64] == NP_TEXT_MAX_TOKENS && text_check_expr(&w.e, 0, 16, why, sizeof why) == 0);
  EXPECT(text_counted_expr_phrases(&w.e, 1, &multi, &prefix) == 64 && multi == 64);
  // the vocabulary bound of the argument-only check: 2^31 passes what a handle's own vocabulary refuses
  Expr far({{2000000000}}, {2000000001});
  EXPECT(text_check_expr(&far.e, 0, (int64_t)1 << 31, why, sizeof why) == 0 && text_check_expr(&far.e, 0, 16, why, sizeof why) != 0);
  EXPECT(text_counted_expr_phrases(&far.e, 1) == 1);
}

static void groups() {
  // a bit per document, whole 256-byte lines; never less than one line
  EXPECT(text_prefix_bitmap_bytes(0) == 256 && text_prefix_bitmap_bytes(-5) == 256 && text_prefix_bitmap_bytes(1) == 256);
  EXPECT(text_prefix_bitmap_bytes(2048) == 256 && text_prefix_bitmap_bytes(2049) == 512);
  for (int64_t n : {1ll, 31ll, 32ll, 33ll, 2047ll, 4096ll, 9001ll, 10000000ll, (1ll << 31) - 1}) {
    const int64_t b = text_prefix_bitmap_bytes(n);
    EXPECT(b % 256 == 0 && b * 8 >= n && (b - 256) * 8 < n);
    EXPECT((n - 1) / 32 < b / 4);   // the word of the last document lies inside the bitmap
    // the scratch the plan leaves is at least one query's frequency arrays: 4 bytes per document, padded to 64 documents
    const int64_t stride = (n + 63) / 64 * 64;
    EXPECT(text_prefix_group(stride * 4, n, 1000) >= 1);
  }
  EXPECT(text_prefix_group(0, 100, 5) == 0 && text_prefix_group(-1, 100, 5) == 0 && text_prefix_group(255, 100, 5) == 0);
  EXPECT(text_prefix_group(256, 100, 5) == 1 && text_prefix_group(1024, 100, 5) == 4 && text_prefix_group(1 << 20, 100, 5) == 5);
  EXPECT(text_prefix_group(1ll << 40, 100, 1 << 20) == 65535);   // the group is a grid dimension
  EXPECT(text_prefix_group(1 << 20, 100, 0) == 0);
  // every phrase is counted exactly once whatever the group
  for (int64_t scratch : {256ll, 1000ll, 4096ll, 1ll << 20})
    for (int64_t n_px : {1ll, 7ll, 64ll, 300ll}) {
      const int64_t g = text_prefix_group(scratch, 2048, n_px);
      int64_t done = 0, calls = 0;
      for (int64_t x0 = 0; x0 < n_px; x0 += g, ++calls) done += g < n_px - x0 ? g : n_px - x0;
      EXPECT(done == n_px && g * text_prefix_bitmap_bytes(2048) <= scratch && calls == (n_px + g - 1) / g);
    }
}

int main() {
  counted_phrases();
  groups();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
