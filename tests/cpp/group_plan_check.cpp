// Stand-alone check of the grouped entry points' host code (next-plaid_amd/csrc/np_group_plan.h: the checks of set_groups and
// of a collapse, the sort width, the LDS bytes, the default pool).  No device, no library: build with the host compiler,
// optionally with -fsanitize=address,undefined, and run.  tests/test_collapse_restate_cpu.py does both.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "np_group_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static bool has(const char* s, const char* part) { return std::strstr(s, part) != nullptr; }

int main() {
  const char* why = nullptr;
  int64_t bad = 0;

  // ---- set_groups ----
  std::vector<int32_t> g = {0, 2, 1, 2, 0};
  EXPECT(group_check_ids(g.data(), 5, 3, 5, 1, &why, &bad) == 0 && bad == -1);
  EXPECT(group_check_ids(g.data(), 5, 3, 5, 0, &why, &bad) == 0);
  EXPECT(group_check_ids(g.data(), 5, 3, 6, 1, &why, &bad) == 1 && has(why, "per document"));   // shape
  EXPECT(group_check_ids(g.data(), 5, 2, 5, 1, &why, &bad) == 2 && bad == 1 && has(why, "outside"));
  g[3] = -1;
  EXPECT(group_check_ids(g.data(), 5, 3, 5, 1, &why, &bad) == 2 && bad == 3);
  g[3] = 2;
  EXPECT(group_check_ids(g.data(), 5, 0, 5, 1, &why, &bad) == 2 && has(why, "n_groups"));
  EXPECT(group_check_ids(g.data(), 5, (int64_t)1 << 31, 5, 1, &why, &bad) == 2 && has(why, "n_groups"));
  EXPECT(group_check_ids(g.data(), 5, ((int64_t)1 << 31) - 1, 5, 1, &why, &bad) == 0);
  EXPECT(group_check_ids(nullptr, 5, 3, 5, 1, &why, &bad) == 2 && has(why, "NULL"));
  EXPECT(group_check_ids(g.data(), -1, 3, 5, 1, &why, &bad) == 2);
  EXPECT(group_check_ids(nullptr, 0, 0, 5, 1, &why, &bad) == 0);          // n = 0 drops, nothing else is looked at
  EXPECT(group_check_ids(g.data(), 5, 3, 5, 2, &why, &bad) == 2 && has(why, "sharded"));
  EXPECT(group_check_ids(nullptr, 0, 0, 5, 2, &why, &bad) == 2 && has(why, "sharded"));
  {
    std::vector<int32_t> top = {0, 0x7FFFFFFE};   // the largest id there is
    EXPECT(group_check_ids(top.data(), 2, NP_GROUP_MAX_GROUPS, 2, 1, &why, &bad) == 0);
    top[1] = 0x7FFFFFFF;
    EXPECT(group_check_ids(top.data(), 2, NP_GROUP_MAX_GROUPS, 2, 1, &why, &bad) == 2 && bad == 1);
  }

  // ---- a collapse's scalars ----
  EXPECT(group_check_args(true, 10, 1, 64, 200, &why) == 0);
  EXPECT(group_check_args(false, 10, 1, 64, 200, &why) == 2 && has(why, "no groups"));
  EXPECT(group_check_args(true, 0, 1, 1, 200, &why) == 2 && has(why, "top_k"));
  EXPECT(group_check_args(true, 1, 0, 1, 200, &why) == 2 && has(why, "group_size"));
  EXPECT(group_check_args(true, 1, 1, -1, 200, &why) == 2);
  EXPECT(group_check_args(true, 1, 1, 0, 200, &why) == 0);
  EXPECT(group_check_args(true, 16384, 1, 1, 1, &why) == 0);
  EXPECT(group_check_args(true, 128, 128, 1, 1, &why) == 0);               // top_k * group_size = 16384
  EXPECT(group_check_args(true, 16385, 1, 1, 1, &why) == 2 && has(why, "16384"));
  EXPECT(group_check_args(true, 5, 3277, 1, 1, &why) == 2 && has(why, "16384"));   // 16385
  EXPECT(group_check_args(true, 0x7FFFFFFF, 0x7FFFFFFF, 1, 1, &why) == 2);  // the product does not wrap
  EXPECT(group_check_args(true, 1, 1, 1, 0, &why) == 2 && has(why, "stride"));
  EXPECT(group_check_args(true, 1, 1, 1, 16384, &why) == 0);
  EXPECT(group_check_args(true, 1, 1, 1, 16385, &why) == 2 && has(why, "stride"));

  // ---- host form: counts and ids ----
  {
    std::vector<int32_t> counts = {3, 0, 4};
    EXPECT(group_first_bad_count(counts.data(), 3, 4) == -1);
    EXPECT(group_first_bad_count(counts.data(), 3, 3) == 2);
    counts[1] = -1;
    EXPECT(group_first_bad_count(counts.data(), 3, 4) == 1);
    counts[1] = 0;
    std::vector<int64_t> ids = {1, 2, 3, 99, /* */ 99, 99, 99, 99, /* */ 0, 4, 4, 1};
    EXPECT(group_first_bad_id(ids.data(), counts.data(), 3, 4, 5) == -1);   // entries past a count are not read
    ids[10] = 5;
    EXPECT(group_first_bad_id(ids.data(), counts.data(), 3, 4, 5) == 10);
    ids[1] = -1;
    EXPECT(group_first_bad_id(ids.data(), counts.data(), 3, 4, 5) == 1);
    EXPECT(group_first_bad_id(ids.data(), counts.data(), 0, 4, 5) == -1);
  }

  // ---- the sort width and the LDS bytes ----
  struct {
    int stride, p2, chunk;
  } shapes[] = {{1, 64, 1}, {64, 64, 1}, {65, 128, 1}, {1023, 1024, 1}, {1024, 1024, 1}, {1025, 2048, 2}, {2049, 4096, 4},
                {16384, 16384, 16}};
  for (const auto& s : shapes) {
    EXPECT(group_p2(s.stride) == s.p2);
    EXPECT(group_chunk(s.stride) == s.chunk);
    EXPECT((int64_t)group_chunk(s.stride) * NP_GROUP_TPB >= s.p2);   // the threads' runs cover every sorted position
    EXPECT(group_lds_bytes(s.stride) == (int64_t)s.p2 * 8 + s.p2 / 8 + s.p2 / 64 * 4 + NP_GROUP_SCAN_WORDS * 4);
    EXPECT(s.p2 / 64 <= NP_GROUP_TPB);                               // one thread per bitmap word
  }
  EXPECT(group_lds_bytes(1) == 512 + 8 + 4 + 128);
  EXPECT(group_lds_bytes(64) == group_lds_bytes(1));
  EXPECT(group_lds_bytes(65) == 1024 + 16 + 8 + 128);
  EXPECT(group_lds_bytes(16384) == 131072 + 2048 + 1024 + 128);
  EXPECT(group_lds_bytes(16384) <= 160 * 1024);                      // a CU's LDS
  EXPECT(NP_GROUP_SCAN_WORDS >= NP_GROUP_TPB / 64);

  // ---- the default pool ----
  EXPECT(group_default_pool(10, 1000000, 16384) == 200);
  EXPECT(group_default_pool(50, 1000000, 16384) == 1000);
  EXPECT(group_default_pool(10, 120, 16384) == 120);
  EXPECT(group_default_pool(10, 3, 16384) == 10);
  EXPECT(group_default_pool(2000, 1000000, 16384) == 16384);
  EXPECT(group_default_pool(200, 1000000, 2048) == 2048);

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
