// Stand-alone check of np_hip_search_exact's host code (next-plaid_amd/csrc/np_scan_plan.h: argument checks, query
// grouping, slice / pass planning).  No device, no library: build with the host compiler, optionally with
// -fsanitize=address,undefined, and run.  tests/test_scan_restate_cpu.py builds and runs it plainly.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "np_scan_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static std::vector<int32_t> offsets(const std::vector<int>& lens) {
  std::vector<int32_t> off(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
  return off;
}

// every query appears once, whole and in order; no group exceeds max(scan_tiles, its only query's tiles)
static void check_groups(const std::vector<int>& lens, int scan_tiles) {
  const std::vector<int32_t> off = offsets(lens);
  const int B = (int)lens.size();
  std::vector<int32_t> info((size_t)(B > 0 ? B : 1) * NP_SCAN_MAX_TILES, 12345);
  int mt = -1, mt2 = -1;
  const int g = scan_pack_groups(off.data(), B, scan_tiles, info.data(), &mt);
  EXPECT(g == scan_pack_groups(off.data(), B, scan_tiles, nullptr, &mt2) && mt == mt2);
  EXPECT(g <= B && (B == 0 || g >= 1) && mt <= NP_SCAN_MAX_TILES);
  int next_q = 0, widest = 0;
  for (int gi = 0; gi < g; ++gi) {
    int used = 0, queries = 0;
    bool ended = false;
    for (int x = 0; x < NP_SCAN_MAX_TILES; ++x) {
      const int32_t v = info[(size_t)gi * NP_SCAN_MAX_TILES + x];
      if (v < 0) {
        ended = true;
        continue;
      }
      EXPECT(!ended);   // used slots are contiguous from 0
      const int b = v & 0xFFFF, t = v >> 16;
      if (t == 0) {
        EXPECT(b == next_q);
        ++next_q;
        ++queries;
      } else {
        EXPECT(b == next_q - 1 && x > 0 && info[(size_t)gi * NP_SCAN_MAX_TILES + x - 1] == (b | ((t - 1) << 16)));
      }
      EXPECT(t < scan_query_tiles(lens[(size_t)b]));
      ++used;
    }
    EXPECT(used >= 1 && (used <= scan_tiles || queries == 1));
    if (used > widest) widest = used;
  }
  EXPECT(next_q == B && (B == 0 || widest == mt));
  int tiles = 0;
  for (int l : lens) tiles += scan_query_tiles(l);
  int listed = 0;
  for (int i = 0; i < g * NP_SCAN_MAX_TILES; ++i) listed += info[(size_t)i] >= 0;
  EXPECT(listed == tiles);
}

int main() {
  // grouping
  const std::vector<std::vector<int>> batches = {
      {}, {1}, {0}, {256}, {1, 33, 256, 48, 32, 64, 200, 5}, {32, 32, 32, 32, 32, 32, 32, 32, 32}, {65, 65, 65, 65},
      {256, 256, 1, 1, 1, 1, 1, 1, 1, 1, 1}, {0, 0, 0}, {31, 225, 1, 255}};
  for (const auto& lens : batches)
    for (int st = 1; st <= NP_SCAN_MAX_TILES; ++st) check_groups(lens, st);
  check_groups({40, 40}, 0);      // clamped to 1
  check_groups({40, 40}, 99);     // clamped to 8
  {
    std::vector<int> many(300);
    for (size_t i = 0; i < many.size(); ++i) many[i] = (int)(i * 37 % 257);
    check_groups(many, 8);
    check_groups(many, 3);
  }
  // argument checks
  const char* why = nullptr;
  const std::vector<int32_t> off = offsets({1, 33, 256});
  EXPECT(scan_check_args(3, 128, 128, true, 10, 0, off.data(), &why) == 0);
  EXPECT(scan_check_args(3, 128, 128, true, 16384, 3, off.data(), &why) == 0);
  EXPECT(scan_check_args(0, 128, 128, true, 1, 0, nullptr, &why) == 0);
  EXPECT(scan_check_args(3, 64, 128, true, 10, 0, off.data(), &why) == 1 && why[0]);
  EXPECT(scan_check_args(3, 160, 160, false, 10, 0, off.data(), &why) == 1 && why[0]);
  EXPECT(scan_check_args(3, 128, 128, true, 0, 0, off.data(), &why) == 2 && why[0]);
  EXPECT(scan_check_args(3, 128, 128, true, 16385, 0, off.data(), &why) == 2);
  EXPECT(scan_check_args(3, 128, 128, true, 10, 1, off.data(), &why) == 2);
  EXPECT(scan_check_args(3, 128, 128, true, 10, 2, off.data(), &why) == 2);
  EXPECT(scan_check_args(3, 128, 128, true, 10, -1, off.data(), &why) == 2);
  EXPECT(scan_check_args(-1, 128, 128, true, 10, 0, off.data(), &why) == 2);
  EXPECT(scan_check_args(70000, 128, 128, true, 10, 0, nullptr, &why) == 2);
  {
    const std::vector<int32_t> bad1 = {1, 2, 3, 4}, bad2 = {0, 5, 3, 4}, bad3 = {0, 257, 258, 259};
    EXPECT(scan_check_args(3, 128, 128, true, 10, 0, bad1.data(), &why) == 1);
    EXPECT(scan_check_args(3, 128, 128, true, 10, 0, bad2.data(), &why) == 1);
    EXPECT(scan_check_args(3, 128, 128, true, 10, 0, bad3.data(), &why) == 1);
  }
  // slices and passes: the plan always fits the budget, covers a document, and honours the knobs
  const int64_t budgets[] = {0, 1000, 1 << 20, 64 << 20, (int64_t)2 << 30, (int64_t)16 << 30};
  const int64_t docs[] = {0, 1, 96, 5000, 10000000};
  for (int64_t budget : budgets)
    for (int64_t nd : docs)
      for (int B : {1, 4, 8, 64, 1000})
        for (int mb : {1, 4, 64})
          for (int64_t sd : {(int64_t)0, (int64_t)17, (int64_t)1 << 20}) {
            const int64_t fixed = 8192, pq = 150000;
            ScanPlan p;
            const bool ok = scan_plan(budget, fixed, pq, nd, B, mb, sd, &p);
            const bool one_fits = budget - fixed - pq >= 8;
            EXPECT(ok == one_fits);
            if (!ok) continue;
            EXPECT(p.S >= 1 && p.S <= B && p.S <= mb && p.P >= 1 && p.P <= (nd < 1 ? 1 : nd));
            EXPECT(fixed + (int64_t)p.S * pq + (int64_t)p.S * p.P * 8 <= budget);
            if (sd > 0) EXPECT(p.P <= sd);
          }
  {
    ScanPlan p;
    EXPECT(scan_plan((int64_t)16 << 30, 0, 150000, 96, 8, 64, 17, &p) && p.S == 8 && p.P == 17);
    EXPECT(scan_plan((int64_t)16 << 30, 0, 150000, 96, 8, 4, 0, &p) && p.S == 4 && p.P == 96);
    EXPECT(scan_plan((int64_t)16 << 30, 0, 150000, 10000000, 64, 64, 0, &p) && p.S == 64 && p.P == 10000000);
    EXPECT(scan_plan((int64_t)1 << 30, 0, 150000, 10000000, 64, 64, 0, &p) && p.S == 64 && p.P < 10000000 && p.P >= 1024);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("scan plan: all checks passed\n");
  return 0;
}
