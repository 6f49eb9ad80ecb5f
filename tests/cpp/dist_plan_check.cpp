// Stand-alone check of the sharded keyword search's host code (next-plaid_amd/csrc/np_dist_plan.h: the record layouts, the
// status words, the rule that cuts a batch into exchanges, the summation and cross-check of the gathered hit counts).  No device,
// no library: build with the host compiler -- tests/test_shard_text_restate_cpu.py builds it plain and with
// -fsanitize=address,undefined -- and run.  Records live in exactly-sized heap buffers: an offset one past the end is a report.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "np_dist_plan.h"

using namespace np;

static int failures = 0;
#define EXPECT(c)                                                \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                \
    }                                                            \
  } while (0)

static void put64(char* at, uint64_t v) { memcpy(at, &v, 8); }

static void status_words() {
  EXPECT(dist_status_word(0, NP_OK) == 0 && dist_status_word(7, NP_OK) == 0);
  const uint64_t w = dist_status_word(2, NP_ERR_INVALID_ARGUMENT);
  EXPECT(w == ((3ull << 32) | (uint32_t)NP_ERR_INVALID_ARGUMENT));
  EXPECT(dist_status_rank(w) == 2 && dist_status_code(w) == NP_ERR_INVALID_ARGUMENT);
  EXPECT(dist_status_rank(0) == -1 && dist_status_code(0) == 0);
  EXPECT(dist_status_rank(dist_status_word(0, NP_ERR_OUT_OF_MEMORY)) == 0);   // rank 0's failure is not "healthy"
}

static void count_records() {
  for (int64_t n : {0ll, 1ll, 5ll, 1000ll}) {
    const DistCountRec r = dist_count_record(n);
    EXPECT(r.n_items == n && r.o_rows == (size_t)n * 8 && r.o_status == r.o_rows + 8 && r.bytes == r.o_status + 8);
    EXPECT(r.bytes % 8 == 0);
  }
  EXPECT(dist_count_record(-3).n_items == 0 && dist_count_record(-3).bytes == 16);
  // three ranks, two counted phrases; every byte of the gathered buffer is written and read
  const DistCountRec r = dist_count_record(2);
  const int G = 3;
  std::unique_ptr<char[]> all(new char[(size_t)G * r.bytes]);
  const uint64_t hits[3][2] = {{4, 0}, {1, 9}, {0, 2}};
  auto fill = [&](const int64_t rows[3], const uint64_t st[3]) {
    for (int g = 0; g < G; ++g) {
      char* rec = all.get() + (size_t)g * r.bytes;
      put64(rec, hits[g][0]);
      put64(rec + 8, hits[g][1]);
      put64(rec + r.o_rows, (uint64_t)rows[g]);
      put64(rec + r.o_status, st[g]);
    }
  };
  std::unique_ptr<uint64_t[]> sums(new uint64_t[2]);
  uint64_t failed = 1;
  int64_t rows = -1;
  int a = -1, b = -1;
  {
    const int64_t rw[3] = {1501, 1501, 1501};
    const uint64_t st[3] = {0, 0, 0};
    fill(rw, st);
    EXPECT(dist_sum_counts(all.get(), r, G, sums.get(), &failed, &rows, &a, &b) == 0);
    EXPECT(sums[0] == 5 && sums[1] == 11 && failed == 0 && rows == 1501);
    EXPECT(dist_first_failure(all.get(), r.bytes, r.o_status, G) == 0);
  }
  {   // different tables: named, whatever the counts
    const int64_t rw[3] = {1501, 1501, 1500};
    const uint64_t st[3] = {0, 0, 0};
    fill(rw, st);
    EXPECT(dist_sum_counts(all.get(), r, G, sums.get(), &failed, &rows, &a, &b) == 1 && a == 0 && b == 2 && failed == 0);
    EXPECT(dist_sum_counts(all.get(), r, G, sums.get(), &failed, &rows, nullptr, nullptr) == 1);
  }
  {   // a failed rank sends no counts and takes no part in the cross-check: its nRow is whatever it is
    const int64_t rw[3] = {1501, 0, 1501};
    const uint64_t st[3] = {0, dist_status_word(1, NP_ERR_INVALID_ARGUMENT), 0};
    fill(rw, st);
    EXPECT(dist_sum_counts(all.get(), r, G, sums.get(), &failed, &rows, &a, &b) == 0);
    EXPECT(sums[0] == 4 && sums[1] == 2 && rows == 1501);
    EXPECT(dist_status_rank(failed) == 1 && dist_status_code(failed) == NP_ERR_INVALID_ARGUMENT);
    EXPECT(dist_first_failure(all.get(), r.bytes, r.o_status, G) == failed);
  }
  {   // nobody healthy
    const int64_t rw[3] = {0, 0, 0};
    const uint64_t st[3] = {dist_status_word(0, 7), dist_status_word(1, 7), dist_status_word(2, 8)};
    fill(rw, st);
    EXPECT(dist_sum_counts(all.get(), r, G, sums.get(), &failed, &rows, &a, &b) == 0);
    EXPECT(sums[0] == 0 && sums[1] == 0 && rows == 0 && dist_status_rank(failed) == 0);
  }
  {   // no counted phrase at all: only nRow and the status cross
    const DistCountRec r0 = dist_count_record(0);
    std::unique_ptr<char[]> two(new char[2 * r0.bytes]);
    for (int g = 0; g < 2; ++g) {
      put64(two.get() + (size_t)g * r0.bytes + r0.o_rows, 9);
      put64(two.get() + (size_t)g * r0.bytes + r0.o_status, 0);
    }
    std::unique_ptr<uint64_t[]> none(new uint64_t[1]);
    EXPECT(dist_sum_counts(two.get(), r0, 2, none.get(), &failed, &rows, &a, &b) == 0 && rows == 9 && failed == 0);
  }
}

static void elig_records() {
  for (int64_t rows : {1ll, 3ll, 12ll})
    for (int64_t words : {2ll, 64ll, 2048ll}) {   // K = 64, 2048, 65536
      const DistEligRec a = dist_elig_record(rows, words, false), b = dist_elig_record(rows, words, true);
      EXPECT(a.bytes == (size_t)(rows * words * 4) && a.o_lens == a.bytes && !a.lens);
      EXPECT(b.o_lens == a.bytes && b.bytes == a.bytes + (size_t)rows * 8 && b.lens);
      EXPECT(b.o_lens % 8 == 0 && b.bytes % 8 == 0);   // i64 lengths, and the OR runs over whole u32 words
    }
  // the last length of the last row ends the record exactly
  const DistEligRec r = dist_elig_record(3, 2, true);
  std::unique_ptr<char[]> rec(new char[r.bytes]);
  memset(rec.get(), 0, r.bytes);
  put64(rec.get() + r.o_lens + 2 * 8, 525);
  uint64_t v;
  memcpy(&v, rec.get() + r.bytes - 8, 8);
  EXPECT(v == 525);
}

static void text_records() {
  for (int B : {1, 2, 3, 12, 65535})
    for (int k : {1, 10, 1024}) {
      const DistTextRec r = dist_text_record(B, k);
      const size_t n = (size_t)B * k;
      EXPECT(r.o_keys == 0 && r.o_ids == n * 8 && r.o_counts == n * 16);
      EXPECT(r.o_status >= r.o_counts + (size_t)B * 4 && r.o_status < r.o_counts + (size_t)B * 4 + 8 && r.o_status % 8 == 0);
      EXPECT(r.bytes == r.o_status + 8);
    }
  // every field of a small record written at its end and read back, in an exactly-sized buffer
  const DistTextRec r = dist_text_record(3, 2);
  std::unique_ptr<char[]> rec(new char[r.bytes]);
  memset(rec.get(), 0, r.bytes);
  put64(rec.get() + r.o_keys + 5 * 8, 11);
  put64(rec.get() + r.o_ids + 5 * 8, 12);
  const int32_t c = 2;
  memcpy(rec.get() + r.o_counts + 2 * 4, &c, 4);
  put64(rec.get() + r.o_status, dist_status_word(4, 2));
  EXPECT(dist_first_failure(rec.get(), r.bytes, r.o_status, 1) == dist_status_word(4, 2));
  EXPECT(r.o_counts + 3 * 4 <= r.o_status);
}

static void exchanges() {
  // the cut depends on B and top_k alone; a record never exceeds the cap unless one query does not fit it (none does:
  // top_k <= 1024 -> 16 KiB per query)
  for (int B : {1, 12, 255, 256, 257, 4096, 65535})
    for (int k : {1, 10, 1023, 1024}) {
      const int q = dist_text_exchange_queries(B, k), n = dist_text_exchanges(B, k);
      EXPECT(q >= 1 && q <= B);
      EXPECT((int64_t)n * q >= B && (int64_t)(n - 1) * q < B);
      EXPECT((int64_t)dist_text_record(q, k).bytes <= NP_DIST_EXCHANGE_BYTES);
      if (q < B) EXPECT((int64_t)dist_text_record(q + 1, k).bytes + 8 > NP_DIST_EXCHANGE_BYTES);   // ... and no smaller than it must be
    }
  EXPECT(dist_text_exchanges(12, 1024) == 1 && dist_text_exchange_queries(12, 1024) == 12);
  EXPECT(dist_text_exchange_queries(65535, 1024) == 255 && dist_text_exchanges(65535, 1024) == 257);
  EXPECT(dist_text_exchanges(0, 10) == 0 && dist_text_exchanges(-1, 10) == 0);
  EXPECT(dist_text_exchange_queries(5, 0) == 5);
}

int main() {
  status_words();
  count_records();
  elig_records();
  text_records();
  exchanges();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all checks passed\n");
  return 0;
}
