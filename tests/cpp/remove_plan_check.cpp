// Stand-alone check of np_hip_index_remove's host code (next-plaid_amd/csrc/np_remove_plan.h: the ids a remove acts on, the
// renumbering, and the slab schedule of the in-place token move).  No device, no library: build with the host compiler --
// tests/test_index_remove_cpu.py builds it with -fsanitize=address,undefined -- and run.  Every schedule is replayed on an
// exactly-sized heap array of rows the way the device runs it (a launch reads all it reads before it writes): the result is
// the compaction, no launch reads a row of the array that it writes itself, and the staging buffer is never exceeded.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "np_remove_plan.h"

namespace {

int failed = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

uint64_t rng_state = 88172645463325252ull;
uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

// replays the plan of (lens, keep) at `slab` on rows of `row` bytes; returns the number of launches
size_t replay(const std::vector<int64_t>& lens, const std::vector<uint8_t>& keep, int64_t row, int64_t slab) {
  const int64_t n = (int64_t)lens.size();
  std::vector<int64_t> off((size_t)n + 1, 0);
  for (int64_t d = 0; d < n; ++d) off[(size_t)d + 1] = off[(size_t)d] + lens[(size_t)d];
  const int64_t T = off[(size_t)n];
  std::vector<uint8_t> tok_keep((size_t)T), a((size_t)(T * row)), want;
  for (int64_t d = 0; d < n; ++d)
    for (int64_t t = off[(size_t)d]; t < off[(size_t)d + 1]; ++t) tok_keep[(size_t)t] = keep[(size_t)d];
  for (size_t i = 0; i < a.size(); ++i) a[i] = (uint8_t)(rnd() >> 11);
  for (int64_t t = 0; t < T; ++t)
    if (tok_keep[(size_t)t]) want.insert(want.end(), a.begin() + t * row, a.begin() + (t + 1) * row);
  const np::RemovePlan p = np::remove_plan(off.data(), keep.data(), n, row, slab);
  CHECK(p.new_tokens * row == (int64_t)want.size());
  CHECK(p.staging_rows <= (slab < 1 ? np::NP_REMOVE_SLAB_DEFAULT : slab) && p.staging_bytes == p.staging_rows * row);
  int64_t first_removed = T;
  for (int64_t d = n - 1; d >= 0; --d)
    if (!keep[(size_t)d] && lens[(size_t)d] > 0) first_removed = off[(size_t)d];
  CHECK(p.first_moved == first_removed);
  std::vector<uint8_t> stage((size_t)(p.staging_rows * row));   // exactly sized: a gather past it is a sanitizer report
  int64_t staged = -1, next_dst = p.first_moved, prev_src1 = p.first_moved;
  for (const np::RemoveLaunch& l : p.launches) {
    std::vector<int64_t> src;
    for (int64_t t = l.src0; t < l.src1; ++t)
      if (tok_keep[(size_t)t]) src.push_back(t);
    CHECK((int64_t)src.size() == l.dst1 - l.dst0 && !src.empty() && src.front() == l.src0 && src.back() + 1 == l.src1);
    CHECK(l.dst0 >= p.first_moved && l.dst1 <= l.src1);
    if (l.mode != np::NP_REMOVE_COPY) {
      CHECK(l.dst0 == next_dst && l.src0 >= prev_src1);   // ascending, without a gap in the destination
      prev_src1 = l.src1;
    }
    std::vector<uint8_t> read;
    for (int64_t t : src) read.insert(read.end(), a.begin() + t * row, a.begin() + (t + 1) * row);
    if (l.mode == np::NP_REMOVE_DIRECT) {
      CHECK(l.dst1 <= l.src0);   // nothing it writes is read by it
      std::copy(read.begin(), read.end(), a.begin() + l.dst0 * row);
      next_dst = l.dst1;
    } else if (l.mode == np::NP_REMOVE_GATHER) {
      CHECK((int64_t)read.size() <= (int64_t)stage.size());
      std::copy(read.begin(), read.end(), stage.begin());
      staged = (int64_t)src.size();
    } else {
      CHECK(l.mode == np::NP_REMOVE_COPY && staged == l.dst1 - l.dst0);
      std::copy(stage.begin(), stage.begin() + staged * row, a.begin() + l.dst0 * row);
      staged = -1;
      next_dst = l.dst1;
    }
  }
  CHECK(next_dst == p.new_tokens || p.launches.empty());
  a.resize(want.size());
  CHECK(a == want);
  return p.launches.size();
}

}  // namespace

int main() {
  // the ids a remove acts on, and the renumbering at a bitmap word's edge
  {
    const int64_t ids[] = {65, 3, -1, 63, 200, 3, 64, 199};
    const std::vector<int64_t> r = np::remove_ids_in_range(ids, 8, 200);
    CHECK((r == std::vector<int64_t>{3, 63, 64, 65, 199}));
    CHECK(np::remove_new_id(r, 0) == 0 && np::remove_new_id(r, 4) == 3 && np::remove_new_id(r, 62) == 61);
    CHECK(np::remove_new_id(r, 66) == 62 && np::remove_new_id(r, 198) == 194);
    CHECK(np::remove_ids_in_range(ids, 0, 200).empty() && np::remove_ids_in_range(nullptr, 0, 5).empty());
  }
  // a one-token removal at the front with a 4500-token survivor behind it: every slab goes through the staging buffer
  {
    const std::vector<int64_t> lens{1, 4500, 3};
    CHECK(replay(lens, {0, 1, 1}, 12, 2000) == 6);
    CHECK(replay(lens, {0, 1, 1}, 64, 1 << 20) == 2);
    CHECK(replay(lens, {0, 1, 1}, 2, 0) == 2);   // the default slab
  }
  // ... and once as many tokens are gone as a slab keeps, the slabs are direct
  CHECK(replay({1, 2000, 4500, 3}, {0, 0, 1, 1}, 12, 2000) == 3);
  CHECK(replay({2000, 2000}, {0, 1}, 4, 2000) == 1);   // d1 == f exactly: direct
  CHECK(replay({3, 4}, {0, 1}, 4, 8) == 2);            // one token short (d1 == f + 1): staged
  // removals only at the end: nothing moves
  CHECK(replay({5, 6, 7, 8}, {1, 1, 0, 0}, 32, 4) == 0);
  CHECK(replay({5, 6, 7, 8}, {1, 1, 1, 1}, 32, 4) == 0);
  CHECK(replay({5, 6, 7, 8}, {0, 0, 0, 0}, 32, 4) == 0);
  CHECK(replay({}, {}, 32, 4) == 0);
  // a slab that holds no survivor: a removed run of 3 slabs between survivors; empty documents on slab edges
  CHECK(replay({4, 30, 4, 0, 0, 2}, {1, 0, 1, 0, 1, 1}, 16, 10) == 1);
  CHECK(replay({0, 10, 0, 10, 0, 10, 0}, {0, 1, 1, 0, 0, 1, 1}, 16, 10) == 1);   // the empty document at the front moves nothing
  CHECK(replay({0, 10, 0}, {0, 1, 0}, 16, 10) == 0);
  // random geometries
  for (int round = 0; round < 300; ++round) {
    const int64_t n = 1 + (int64_t)(rnd() % 60);
    std::vector<int64_t> lens((size_t)n);
    std::vector<uint8_t> keep((size_t)n);
    const uint64_t odds = 1 + rnd() % 9;
    for (int64_t d = 0; d < n; ++d) {
      lens[(size_t)d] = rnd() % 4 == 0 ? 0 : (int64_t)(rnd() % 40);
      keep[(size_t)d] = rnd() % 10 < odds;
    }
    (void)replay(lens, keep, 1 + (int64_t)(rnd() % 24), 1 + (int64_t)(rnd() % 64));
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
