// Stand-alone check of np_hip_score_pairs' host code (next-plaid_amd/csrc/np_pairs_plan.h: argument checks, row offsets,
// the workgroup map, query slices, staging chunks and the budget plan).  No device, no library: build with the host
// compiler, optionally with -fsanitize=address,undefined, and run.  tests/test_pairs_restate_cpu.py does both.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "np_pairs_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

template <class T, class U>
static std::vector<T> offsets(const std::vector<U>& lens) {
  std::vector<T> off(lens.size() + 1, 0);
  for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + (T)lens[i];
  return off;
}

// the map and the row offsets of one batch cut into slices of S: every workgroup finds its query, every pair is covered
// once, and the row of pair p of query i starts where the header says
static void check_map(const std::vector<int>& lq, const std::vector<int64_t>& np_, int S) {
  const int B = (int)lq.size();
  const std::vector<int32_t> qoff = offsets<int32_t>(lq);
  const std::vector<int64_t> poff = offsets<int64_t>(np_);
  std::vector<int64_t> want_row(B + 1, 0);
  for (int i = 0; i < B; ++i) want_row[i + 1] = want_row[i] + np_[i] * lq[i];
  EXPECT(pairs_rows(qoff.data(), poff.data(), B) == want_row[B]);
  int64_t row0 = 0;
  int covered = 0;
  for (int s0 = 0; s0 < B;) {
    int ml = -1;
    const int Sn = pairs_next_slice(qoff.data(), poff.data(), s0, B, S, &ml);
    EXPECT(Sn >= 1 && Sn <= S && s0 + Sn <= B);
    if (Sn < 1) return;
    int want_ml = 0;
    for (int i = 0; i < Sn; ++i) want_ml = lq[s0 + i] > want_ml ? lq[s0 + i] : want_ml;
    EXPECT(ml == want_ml);
    std::vector<int32_t> wgpre(Sn + 1, -7);
    std::vector<int64_t> rowbase(Sn + 1, -7);
    const int64_t wgs = pairs_prefix(qoff.data() + s0, poff.data() + s0, Sn, wgpre.data(), rowbase.data());
    EXPECT(wgs == pairs_prefix(qoff.data() + s0, poff.data() + s0, Sn, nullptr, nullptr));
    EXPECT(wgpre[0] == 0 && wgpre[Sn] == wgs && rowbase[0] == 0);
    std::vector<int64_t> seen(Sn, 0);
    for (int64_t wg = 0; wg < wgs; ++wg) {
      const int i = pairs_query_of(wgpre.data(), Sn, wg);
      EXPECT(i >= 0 && i < Sn && wgpre[i] <= wg && wg < wgpre[i + 1]);
      const int64_t first = (wg - wgpre[i]) * NP_PAIRS_WG_DOCS;
      EXPECT(first < np_[s0 + i]);
      const int64_t left = np_[s0 + i] - first;
      seen[i] += left < NP_PAIRS_WG_DOCS ? left : NP_PAIRS_WG_DOCS;
    }
    for (int i = 0; i < Sn; ++i) {
      EXPECT(seen[i] == np_[s0 + i]);
      EXPECT(row0 + rowbase[i] == want_row[s0 + i]);
    }
    row0 += pairs_rows(qoff.data() + s0, poff.data() + s0, Sn);
    EXPECT(row0 == want_row[s0 + Sn]);
    s0 += Sn;
    covered += Sn;
  }
  EXPECT(covered == B && row0 == want_row[B]);
}

// chunks under `cap` bytes: they tile the pair list and the rows in order, each fits, each is as large as it may be
static void check_chunks(const std::vector<int>& lq, const std::vector<int64_t>& np_, bool rows, int64_t cap) {
  const int B = (int)lq.size();
  const std::vector<int32_t> qoff = offsets<int32_t>(lq);
  const std::vector<int64_t> poff = offsets<int64_t>(np_);
  const int64_t P = B ? poff[B] : 0, R = rows ? pairs_rows(qoff.data(), poff.data(), B) : 0;
  int worst = 0;
  for (int i = 0; i < B; ++i)
    if (np_[i] > 0 && lq[i] > worst) worst = lq[i];
  const bool fits = cap >= pairs_pair_bytes(worst, rows);
  PairsChunk c;
  int64_t p0 = 0, r0 = 0;
  int hint = 0, n = 0;
  while (pairs_next_chunk(qoff.data(), poff.data(), B, rows, cap, hint, p0, r0, &c)) {
    EXPECT(c.p0 == p0 && c.r0 == r0 && c.p1 > c.p0 && c.p1 <= P && c.q0 < c.q1 && c.q1 <= B);
    EXPECT(poff[c.q0] <= c.p0 && c.p0 < poff[c.q0 + 1]);          // q0 owns the first pair
    EXPECT(poff[c.q1 - 1] < c.p1 && c.p1 <= poff[c.q1]);           // q1 - 1 owns the last
    int64_t bytes = 0, r = 0;
    for (int q = c.q0; q < c.q1; ++q) {
      const int64_t lo = poff[q] > c.p0 ? poff[q] : c.p0, hi = poff[q + 1] < c.p1 ? poff[q + 1] : c.p1;
      if (hi > lo) {
        bytes += (hi - lo) * pairs_pair_bytes(lq[q], rows);
        r += rows ? (hi - lo) * lq[q] : 0;
      }
    }
    EXPECT(bytes <= cap && c.r1 - c.r0 == r);
    if (c.p1 < P) {   // greedy: the next pair would not have fitted
      int q = c.q1 - 1;
      while (poff[q + 1] <= c.p1) ++q;
      EXPECT(bytes + pairs_pair_bytes(lq[q], rows) > cap);
    }
    p0 = c.p1;
    r0 = c.r1;
    hint = c.q1 - 1;
    if (++n > 1000000) break;
  }
  if (fits) EXPECT(p0 == P && r0 == R);
  else EXPECT(p0 < P || P == 0);
}

int main() {
  const std::vector<std::pair<std::vector<int>, std::vector<int64_t>>> batches = {
      {{}, {}},
      {{5}, {0}},
      {{5}, {1}},
      {{1, 33, 256}, {16, 17, 15}},
      {{33, 0, 200, 7}, {40, 3, 0, 1000}},
      {{32, 32, 32, 32, 32}, {0, 0, 5, 0, 0}},
      {{256, 1, 64, 65, 31}, {1, 1, 1, 1, 1}},
      {{3, 4, 5, 6, 7, 8, 9, 10, 11}, {100, 0, 33, 16, 32, 1, 0, 0, 250}},
  };
  for (const auto& b : batches)
    for (int S : {1, 2, 3, 4, 64}) check_map(b.first, b.second, S);
  for (const auto& b : batches)
    for (bool rows : {false, true})
      for (int64_t cap : {(int64_t)0, (int64_t)11, (int64_t)12, (int64_t)100, (int64_t)2059, (int64_t)2060, (int64_t)5000,
                          (int64_t)100000, (int64_t)1 << 30})
        check_chunks(b.first, b.second, rows, cap);
  {   // a chunk may end inside a query's list, and the next starts there
    const std::vector<int> lq = {4, 4};
    const std::vector<int64_t> np_ = {5, 5};
    const auto qoff = offsets<int32_t>(lq);
    const auto poff = offsets<int64_t>(np_);
    PairsChunk c;
    EXPECT(pairs_next_chunk(qoff.data(), poff.data(), 2, true, 44 * 3, 0, 0, 0, &c) && c.p1 == 3 && c.q0 == 0 && c.q1 == 1 && c.r1 == 12);
    EXPECT(pairs_next_chunk(qoff.data(), poff.data(), 2, true, 44 * 3, 0, 3, 12, &c) && c.p1 == 6 && c.q0 == 0 && c.q1 == 2 && c.r1 == 24);
    EXPECT(pairs_next_chunk(qoff.data(), poff.data(), 2, true, 44 * 30, 1, 6, 24, &c) && c.p1 == 10 && c.q0 == 1 && c.q1 == 2 && c.r1 == 40);
    EXPECT(!pairs_next_chunk(qoff.data(), poff.data(), 2, true, 44 * 30, 1, 10, 40, &c));
  }
  // a slice never exceeds a one-dimensional grid
  {
    const std::vector<int> lq = {1, 1, 1};
    const std::vector<int64_t> np_ = {NP_PAIRS_MAX_GRID * (int64_t)NP_PAIRS_WG_DOCS, 16, 1};
    const auto qoff = offsets<int32_t>(lq);
    const auto poff = offsets<int64_t>(np_);
    EXPECT(pairs_next_slice(qoff.data(), poff.data(), 0, 3, 64, nullptr) == 1);
    EXPECT(pairs_next_slice(qoff.data(), poff.data(), 1, 3, 64, nullptr) == 2);
    EXPECT(pairs_query_wgs(0) == 0 && pairs_query_wgs(1) == 1 && pairs_query_wgs(16) == 1 && pairs_query_wgs(17) == 2);
  }
  // argument checks
  const char* why = nullptr;
  const auto qoff = offsets<int32_t>(std::vector<int>{1, 33, 256});
  const auto poff = offsets<int64_t>(std::vector<int64_t>{3, 0, 2});
  EXPECT(pairs_check_args(3, 128, 128, true, 0, qoff.data(), poff.data(), &why) == 0 && !why[0]);
  EXPECT(pairs_check_args(0, 128, 128, true, 0, nullptr, nullptr, &why) == 0);
  EXPECT(pairs_check_args(-1, 128, 128, true, 0, qoff.data(), poff.data(), &why) == 2 && why[0]);
  EXPECT(pairs_check_args(3, 64, 128, true, 0, qoff.data(), poff.data(), &why) == 1 && why[0]);
  EXPECT(pairs_check_args(3, 160, 160, false, 0, qoff.data(), poff.data(), &why) == 1 && why[0]);
  for (int prec : {1, 2, 3, 4, -1}) EXPECT(pairs_check_args(3, 128, 128, true, prec, qoff.data(), poff.data(), &why) == 2 && why[0]);
  EXPECT(pairs_check_args(3, 128, 128, true, 0, nullptr, poff.data(), &why) == 2);
  EXPECT(pairs_check_args(3, 128, 128, true, 0, qoff.data(), nullptr, &why) == 2);
  {
    const std::vector<int32_t> q1 = {1, 2, 3, 4}, q2 = {0, 5, 3, 4}, q3 = {0, 257, 258, 259};
    EXPECT(pairs_check_args(3, 128, 128, true, 0, q1.data(), poff.data(), &why) == 1);
    EXPECT(pairs_check_args(3, 128, 128, true, 0, q2.data(), poff.data(), &why) == 1);
    EXPECT(pairs_check_args(3, 128, 128, true, 0, q3.data(), poff.data(), &why) == 1 && why[0]);
    const std::vector<int64_t> p1 = {1, 3, 3, 5}, p2 = {0, 3, 2, 5},
                               p3 = {0, 0, 0, (NP_PAIRS_MAX_GRID + 1) * (int64_t)NP_PAIRS_WG_DOCS};
    EXPECT(pairs_check_args(3, 128, 128, true, 0, qoff.data(), p1.data(), &why) == 2 && why[0]);
    EXPECT(pairs_check_args(3, 128, 128, true, 0, qoff.data(), p2.data(), &why) == 2 && why[0]);
    EXPECT(pairs_check_args(3, 128, 128, true, 0, qoff.data(), p3.data(), &why) == 2 && why[0]);
  }
  {
    const std::vector<int64_t> ids = {0, 95, 7, 96, -1};
    EXPECT(pairs_first_bad_id(ids.data(), 3, 96) == -1);
    EXPECT(pairs_first_bad_id(ids.data(), 5, 96) == 3);
    EXPECT(pairs_first_bad_id(ids.data() + 4, 1, 96) == 0);
    EXPECT(pairs_first_bad_id(ids.data(), 0, 96) == -1);
  }
  // the budget plan: fits, honours max_batch, refuses what cannot hold one query and one pair
  for (int64_t budget : {(int64_t)0, (int64_t)1000, (int64_t)200000, (int64_t)1 << 20, (int64_t)64 << 20, (int64_t)16 << 30})
    for (int B : {1, 4, 8, 64, 1000})
      for (int mb : {1, 4, 64})
        for (int64_t worst : {(int64_t)0, (int64_t)12, (int64_t)2060}) {
          const int64_t fixed = 8192, pq = 131088;
          PairsPlan p;
          const bool ok = pairs_plan(budget, fixed, pq, B, mb, worst, &p);
          EXPECT(ok == (budget - fixed - pq >= worst));
          if (!ok) continue;
          EXPECT(p.S >= 1 && p.S <= B && p.S <= mb);
          EXPECT(fixed + (int64_t)p.S * pq + p.chunk <= budget && p.chunk <= NP_PAIRS_MAX_CHUNK);
          EXPECT(worst == 0 ? p.chunk == 0 : p.chunk >= worst);
        }
  {
    PairsPlan p;
    EXPECT(pairs_plan((int64_t)16 << 30, 0, 131088, 8, 64, 2060, &p) && p.S == 8 && p.chunk == NP_PAIRS_MAX_CHUNK);
    EXPECT(pairs_plan((int64_t)16 << 30, 0, 131088, 8, 4, 2060, &p) && p.S == 4);
    EXPECT(pairs_plan(400000, 0, 131088, 8, 64, 2060, &p) && p.S == 2 && p.chunk == 400000 - 2 * 131088);
  }
  if (failures) {
    std::printf("%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("pairs plan: all checks passed\n");
  return 0;
}
