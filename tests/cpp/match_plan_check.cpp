// Stand-alone check of the text matcher's host code (next-plaid_amd/csrc/np_match_plan.h: the checks of a packed DFA, its
// device image and the chunk plan).  No device, no library: build with the host compiler -- tests/test_regex_restate_cpu.py
// builds it plain and with -fsanitize=address,undefined -- and run.  Every table lives in an exactly-sized heap buffer, so a
// read past it is a sanitizer report.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "np_match_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

struct Table {
  int64_t ns, nc;
  uint32_t start = 0;
  std::vector<uint8_t> class_of, flags;
  std::vector<uint16_t> table;
  Table(int64_t ns_, int64_t nc_) : ns(ns_), nc(nc_), class_of(256, 0), flags((size_t)ns_, 0), table((size_t)(ns_ * nc_), 0) {
    for (int b = 0; b < 256; ++b) class_of[b] = (uint8_t)(b % nc);
    for (int64_t s = 0; s < ns; ++s)
      for (int64_t c = 0; c < nc; ++c) table[(size_t)(s * nc + c)] = (uint16_t)((s + c + 1) % ns);   // a ring: no absorbing state
  }
  template <class W>
  std::unique_ptr<W[]> pack(int64_t* n_words) const {
    const int64_t n = match_dfa_words(ns, nc);
    std::unique_ptr<W[]> w(new W[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) w[i] = 0;
    w[0] = (W)NP_DFA_MAGIC;
    w[1] = (W)ns;
    w[2] = (W)nc;
    w[3] = (W)start;
    for (int b = 0; b < 256; ++b) w[4 + b / 4] |= (W)class_of[b] << (8 * (b & 3));
    const int64_t f0 = NP_DFA_HEADER_WORDS, t0 = f0 + (ns + 3) / 4;
    for (int64_t s = 0; s < ns; ++s) w[f0 + s / 4] |= (W)flags[(size_t)s] << (8 * (s & 3));
    for (int64_t e = 0; e < ns * nc; ++e) w[t0 + e / 2] |= (W)table[(size_t)e] << (16 * (e & 1));
    *n_words = n;
    return w;
  }
};

static std::string last;
template <class W>
static int check(const Table& t, MatchDfaInfo* info = nullptr, int64_t drop_words = 0) {
  int64_t n = 0;
  auto w = t.pack<W>(&n);
  std::unique_ptr<W[]> exact(new W[(size_t)(n - drop_words)]);   // exactly the words handed over
  memcpy(exact.get(), w.get(), (size_t)(n - drop_words) * sizeof(W));
  char why[160] = "";
  const int rc = match_check_dfa(exact.get(), n - drop_words, 7, why, sizeof why, info);
  last = why;
  return rc;
}
static bool says(const char* what) { return last.find(what) != std::string::npos; }

static void well_formed() {
  const int64_t shapes[][2] = {{1, 1}, {1, 256}, {4096, 1}, {4096, 256}, {3, 5}, {5, 3}, {7, 7}};
  for (const auto& sh : shapes) {
    Table t(sh[0], sh[1]);
    t.start = (uint32_t)(sh[0] - 1);
    t.flags[0] = sh[0] == 1 ? 0 : NP_DFA_ACCEPT_AT_END;
    MatchDfaInfo info;
    EXPECT(check<uint32_t>(t, &info) == 0);
    EXPECT(check<int64_t>(t) == 0);
    EXPECT(info.n_states == sh[0] && info.n_classes == sh[1] && info.start == sh[0] - 1);
    EXPECT(info.image_bytes == ((256 + sh[0] * sh[1] * 2 + 15) & ~15LL));
    // the image: entries carry the target's flags, nothing is written past image_bytes
    int64_t n = 0;
    auto w = t.pack<uint32_t>(&n);
    std::unique_ptr<uint8_t[]> image(new uint8_t[(size_t)info.image_bytes]);
    const uint32_t start = match_build_image(w.get(), info, image.get());
    EXPECT((start & NP_MATCH_E_STATE) == (uint32_t)(sh[0] - 1));
    for (int b = 0; b < 256; ++b) EXPECT(image[b] == t.class_of[b]);
    for (int64_t e = 0; e < sh[0] * sh[1]; e += 97) {
      uint16_t v;
      memcpy(&v, image.get() + 256 + 2 * e, 2);
      EXPECT((v & NP_MATCH_E_STATE) == t.table[(size_t)e]);
      EXPECT(((v & NP_MATCH_E_ACCEPT) != 0) == ((t.flags[t.table[(size_t)e]] & NP_DFA_ACCEPT_AT_END) != 0));
      EXPECT(!(v & (NP_MATCH_E_DEAD | NP_MATCH_E_MATCHED)));
    }
  }
  // absorbing states as the compilers emit them
  Table t(3, 2);
  t.flags = {0, NP_DFA_ACCEPT_AT_END | NP_DFA_MATCHED, NP_DFA_DEAD};
  t.table = {1, 2, 1, 1, 2, 2};
  MatchDfaInfo info;
  EXPECT(check<uint32_t>(t, &info) == 0);
  int64_t n = 0;
  auto w = t.pack<int64_t>(&n);
  std::unique_ptr<uint8_t[]> image(new uint8_t[(size_t)info.image_bytes]);
  EXPECT(match_build_image(w.get(), info, image.get()) == 0u);
  uint16_t v[2];
  memcpy(v, image.get() + 256, 4);
  EXPECT(v[0] == (1u | NP_MATCH_E_ACCEPT | NP_MATCH_E_MATCHED) && v[1] == (2u | NP_MATCH_E_DEAD));
}

static void one_rule_each() {
  {  // a transition one past the last state, in the last entry
    Table t(5, 3);
    t.table.back() = 5;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("DFA 7, state 4") && says("not below n_states"));
    EXPECT(check<int64_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 4"));
  }
  {  // 4096 states, a transition to 4096
    Table t(4096, 2);
    t.table[2 * 4000 + 1] = 4096;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 4000"));
  }
  {  // a class one past the last class, for the last byte
    Table t(2, 256);
    Table u(2, 255);
    u.class_of[255] = 255;
    EXPECT(check<uint32_t>(t) == 0);
    EXPECT(check<uint32_t>(u) == NP_ERR_INVALID_ARGUMENT && says("class of byte 255"));
  }
  {  // MATCHED and DEAD rows point to themselves
    Table t(3, 2);
    t.flags = {0, NP_DFA_ACCEPT_AT_END | NP_DFA_MATCHED, NP_DFA_DEAD};
    t.table = {1, 2, 1, 0, 2, 2};
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 1") && says("point to itself"));
    t.table = {1, 2, 1, 1, 2, 1};
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 2") && says("point to itself"));
    t.table = {1, 2, 1, 1, 2, 2};
    t.flags[1] = NP_DFA_MATCHED;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 1") && says("MATCHED without ACCEPT_AT_END"));
    t.flags[1] = NP_DFA_ACCEPT_AT_END | NP_DFA_MATCHED;
    t.flags[2] = NP_DFA_DEAD | NP_DFA_ACCEPT_AT_END;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 2") && says("DEAD with ACCEPT_AT_END"));
    t.flags[2] = 8;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("state 2") && says("unknown flag"));
  }
  {  // sizes
    Table t(6, 3);
    EXPECT(check<uint32_t>(t, nullptr, 1) == NP_ERR_INVALID_ARGUMENT && says("n_words"));
    t.start = 6;
    EXPECT(check<uint32_t>(t) == NP_ERR_INVALID_ARGUMENT && says("start state"));
    int64_t n = 0;
    Table ok(6, 3);
    auto w = ok.pack<uint32_t>(&n);
    char why[160];
    auto with = [&](int word, uint32_t v) {
      std::unique_ptr<uint32_t[]> c(new uint32_t[(size_t)n]);
      memcpy(c.get(), w.get(), (size_t)n * 4);
      c[word] = v;
      const int rc = match_check_dfa(c.get(), n, 0, why, sizeof why, nullptr);
      last = why;
      return rc;
    };
    EXPECT(with(0, 1) == NP_ERR_INVALID_ARGUMENT && says("magic"));
    EXPECT(with(1, 0) == NP_ERR_INVALID_ARGUMENT && says("n_states"));
    EXPECT(with(1, 4097) == NP_ERR_INVALID_ARGUMENT && says("n_states"));
    EXPECT(with(2, 0) == NP_ERR_INVALID_ARGUMENT && says("n_classes"));
    EXPECT(with(2, 257) == NP_ERR_INVALID_ARGUMENT && says("n_classes"));
    EXPECT(with(1, 7) == NP_ERR_INVALID_ARGUMENT && says("n_words"));   // more states than the words hold: refused, not read
    std::unique_ptr<uint32_t[]> tiny(new uint32_t[3]{NP_DFA_MAGIC, 1, 1});
    EXPECT(match_check_dfa(tiny.get(), 3, 0, why, sizeof why, nullptr) == NP_ERR_INVALID_ARGUMENT);
    EXPECT(match_check_dfa((const uint32_t*)nullptr, 70, 0, why, sizeof why, nullptr) == NP_ERR_INVALID_ARGUMENT);
    // an i64 value that is no 32-bit word
    auto w64 = ok.pack<int64_t>(&n);
    w64[n - 1] |= (int64_t)1 << 32;
    EXPECT(match_check_dfa(w64.get(), n, 0, why, sizeof why, nullptr) == NP_ERR_INVALID_ARGUMENT && strstr(why, "32 bits"));
    w64[n - 1] = -1;
    EXPECT(match_check_dfa(w64.get(), n, 0, why, sizeof why, nullptr) == NP_ERR_INVALID_ARGUMENT);
  }
}

static void plans() {
  const int64_t counts[] = {0, 1, 64, 65, 255, 256, 257, 10000000};
  const int64_t images[3] = {512, 2 * 1024 * 1024 + 256, 4096};
  for (int64_t n : counts)
    for (int32_t nd = 1; nd <= 3; ++nd) {
      int64_t sum = 0, largest = 0;
      for (int i = 0; i < nd; ++i) {
        sum += images[i];
        largest = std::max(largest, images[i]);
      }
      const int64_t budgets[] = {0, 4096, largest + 4096 + 31, largest + 4096 + 32, sum + 4096 + nd * 32 - 1, sum + 4096 + nd * 32,
                                 sum + 4096 + nd * 32 * 5, sum + 4096 + nd * (n / 8 + 64), (int64_t)1 << 34};
      for (int64_t budget : budgets) {
        MatchPlan p;
        const bool ok = match_plan(budget, images, nd, n, NP_MATCH_LDS_TABLE_BYTES, &p);
        EXPECT(ok == (budget >= largest + 4096 + 32));   // too small: the caller returns NP_ERR_OUT_OF_MEMORY
        if (!ok) continue;
        EXPECT(p.dfas == nd || p.dfas == 1);
        EXPECT(p.dfas == nd || budget < sum + 4096 + nd * 32);
        EXPECT(p.strings >= 1 && (p.strings % NP_MATCH_BLOCK_STRINGS == 0 || p.strings == std::max<int64_t>(n, 1)));
        EXPECT(p.scratch_bytes() <= budget);
        EXPECT(p.tile_bytes % 16 == 0 && p.tile_bytes + 256 + p.table_lds_bytes <= 64 * 1024);
        // every (DFA, string) exactly once, in whole blocks
        int64_t covered = 0, groups = 0;
        for (int32_t d0 = 0; d0 < nd; d0 += p.dfas) {
          ++groups;
          int64_t next = 0;
          for (int64_t s0 = 0; s0 < n; s0 += p.strings) {
            EXPECT(s0 == next && s0 % NP_MATCH_BLOCK_STRINGS == 0);
            next = s0 + std::min(p.strings, n - s0);
            covered += (next - s0) * std::min<int64_t>(p.dfas, nd - d0);
          }
          EXPECT(next == n);
        }
        EXPECT(covered == n * nd && groups == (nd + p.dfas - 1) / p.dfas);
      }
    }
  MatchPlan p;
  EXPECT(p.table_in_lds(256 + NP_MATCH_LDS_TABLE_BYTES) && !p.table_in_lds(256 + NP_MATCH_LDS_TABLE_BYTES + 16));
  EXPECT(NP_MATCH_TILE_BYTES + 256 + NP_MATCH_LDS_TABLE_MAX <= 64 * 1024);
  EXPECT(NP_MATCH_MAX_STRING_BYTES == 256 * (int64_t)NP_MATCH_TILE_BYTES);   // a long string costs its block at most 256 tiles
}

int main() {
  well_formed();
  one_rule_each();
  plans();
  if (failures) {
    std::printf("%d checks FAILED\n", failures);
    return 1;
  }
  std::printf("match plan check ok\n");
  return 0;
}
