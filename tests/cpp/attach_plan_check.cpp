// np_attach_plan.h stand-alone, with the host compiler: the select of a survivor's source against a plain scan over the keep
// flags at the document counts and keep patterns the GPU test uses, the k-th set bit against a loop over the bits, the tail
// merge word and the remap check.  Built under ASan + UBSan by tests/test_attach_restate_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../next-plaid_amd/csrc/np_attach_plan.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static void check_select(const std::vector<uint8_t>& keep) {
  const int64_t n = (int64_t)keep.size(), W = (n + 63) / 64;
  std::vector<uint64_t> bits((size_t)W, 0);
  std::vector<uint32_t> wrank((size_t)W, 0);
  uint32_t gone = 0;
  for (int64_t w = 0; w < W; ++w) {
    for (int b = 0; b < 64; ++b)
      if (64 * w + b >= n || keep[(size_t)(64 * w + b)]) bits[(size_t)w] |= (uint64_t)1 << b;
    wrank[(size_t)w] = gone;
    gone += 64u - (uint32_t)np::attach_popc64(bits[(size_t)w]);
  }
  int64_t j = 0;
  for (int64_t d = 0; d < n; ++d)
    if (keep[(size_t)d]) {
      CHECK(np::attach_select(bits.data(), wrank.data(), W, j) == d);
      ++j;
    }
}

int main() {
  // the k-th set bit of a word, against a loop
  uint64_t x = 0x9E3779B97F4A7C15ull;
  for (int r = 0; r < 200; ++r) {
    x ^= x << 13, x ^= x >> 7, x ^= x << 17;
    const uint64_t words[4] = {x, x & (x >> 1), ~(uint64_t)0, (uint64_t)1 << (r % 64)};
    for (uint64_t w : words) {
      int k = 0;
      for (int b = 0; b < 64; ++b)
        if ((w >> b) & 1) CHECK(np::attach_select_bit(w, k++) == b);
    }
  }
  // the select over whole bitmaps
  const int64_t sizes[] = {1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097, 32769};
  for (int64_t n : sizes) {
    std::vector<uint8_t> keep((size_t)n, 1);
    check_select(keep);   // none removed
    keep[0] = 0;
    check_select(keep);   // the first
    keep[0] = 1, keep[(size_t)n - 1] = 0;
    check_select(keep);   // the last
    for (int64_t d = 0; d < n; ++d) keep[(size_t)d] = (uint8_t)(d & 1);
    check_select(keep);   // every other
    for (int64_t d = 0; d < n; ++d) keep[(size_t)d] = (uint8_t)(d == n / 2);
    check_select(keep);   // all but one
    for (int64_t d = 0; d < n; ++d) keep[(size_t)d] = (uint8_t)(d >= (n - 1) / 64 * 64);
    check_select(keep);   // survivors only in the last word
    for (int64_t d = 0; d < n; ++d) keep[(size_t)d] = (uint8_t)!(d >= 64 && d < 128);
    check_select(keep);   // one whole word
    for (int64_t d = 0; d < n; ++d) keep[(size_t)d] = (uint8_t)!(d >= 70 && d < 400);
    check_select(keep);   // a removed run longer than 256
    for (int64_t d = 0; d < n; ++d) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      keep[(size_t)d] = (uint8_t)(x % 10 != 0);
    }
    check_select(keep);   // a random tenth
  }
  // the wave's ballot as two words
  CHECK(np::attach_ballot_word(0x0123456789ABCDEFull, 0) == 0x89ABCDEFu && np::attach_ballot_word(0x0123456789ABCDEFull, 1) == 0x01234567u);
  // the tail merge: old bits kept, new bits OR-ed in, what lay past the old count not trusted; a fresh bitmap's old rows are valid
  CHECK(np::attach_merge_word(0x0000FFFFu, 0xA5A50000u, 16, false) == 0xA5A5FFFFu);
  CHECK(np::attach_merge_word(0xDEAD00F0u, 0x00010000u, 8, false) == 0x000100F0u);
  CHECK(np::attach_merge_word(0u, 0x80000000u, 31, true) == 0xFFFFFFFFu);
  CHECK(np::attach_merge_word(0x12345678u, 0x0000000Fu, 0, false) == 0x0000000Fu);
  CHECK(np::attach_merge_word(0u, 0xFFFE0000u, 17, true) == 0xFFFFFFFFu);
  // remaps
  const int32_t good[] = {0, 2, 3, 7}, flat[] = {0, 2, 2, 7}, down[] = {1, 0}, neg[] = {-1, 0};
  CHECK(np::attach_remap_check(good, 4) == -1 && np::attach_remap_check(good, 0) == -1);
  CHECK(np::attach_remap_check(flat, 4) == 2 && np::attach_remap_check(down, 2) == 1 && np::attach_remap_check(neg, 2) == 0);
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
