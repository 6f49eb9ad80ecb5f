// np_attach_plan.h -- the select rule of the attachment compaction (np_index.hip attach_compact_kernel): where the document
// that gets NEW id j lies among the old ones, from the keep bitmap of a remove (one u64 per 64 old documents, bit = the document
// stays, bits past n_docs set) and the removed documents in front of each word.  The same functions run in the kernel and on
// the host; tests/cpp/attach_plan_check.cpp runs them stand-alone.
//
// The kept documents in front of word w are 64 w - wrank[w]: monotone in w, so the word of new id j is a bisection, and the
// document inside it is the (j - kept in front)-th set bit of the word.  The phantom bits past n_docs lie behind every real
// document of the last word, so an id below the number of survivors never selects one.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define NP_ATTACH_HD __host__ __device__ inline
#else
#define NP_ATTACH_HD inline
#endif

namespace np {

NP_ATTACH_HD int attach_popc64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// the word that holds the survivor with new id j (j < survivors): the first w in [0, n_words - 1) with more than j kept
// documents up to its end (64 (w + 1) - wrank[w + 1] >= j + 1: a lower bound), or the last word
NP_ATTACH_HD int64_t attach_select_word(const uint32_t* wrank, int64_t n_words, int64_t j) {
  int64_t a = 0, z = n_words - 1;
  while (a < z) {
    const int64_t mid = (a + z) >> 1;
    if (64 * (mid + 1) - (int64_t)wrank[mid + 1] < j + 1) a = mid + 1;
    else z = mid;
  }
  return a;
}

// the position of the k-th set bit of word (k counts from 0 and is below the word's popcount): by halves, no loop over bits
NP_ATTACH_HD int attach_select_bit(uint64_t word, int k) {
  int pos = 0;
  for (int s = 32; s > 0; s >>= 1) {
    const int c = attach_popc64(word & (((uint64_t)1 << s) - 1));
    if (k >= c) {
      k -= c;
      word >>= s;
      pos += s;
    }
  }
  return pos;
}

// the old id of the survivor with new id j
NP_ATTACH_HD int64_t attach_select(const uint64_t* bits, const uint32_t* wrank, int64_t n_words, int64_t j) {
  const int64_t w = attach_select_word(wrank, n_words, j);
  return 64 * w + attach_select_bit(bits[w], (int)(j - (64 * w - (int64_t)wrank[w])));
}

// a wave's 64 validity bits (lane l = bit l) as the two u32 words of a column's bitmap: word 0 is the wave's first 32 documents
NP_ATTACH_HD uint32_t attach_ballot_word(uint64_t ballot, int half) { return (uint32_t)(ballot >> (32 * half)); }

// An append's validity tail.  The new rows' bits are laid out at their final positions, so their first word is the word that
// holds the old last document when the old count is no multiple of 32: `shared_bits` = old count & 31 of its bits belong to old
// rows.  That word is MERGED -- the old rows' bits kept (all ones where the column had no bitmap: fresh), the new ones OR-ed in;
// whatever lay past the old count is not trusted -- and every later word is the tail's.
NP_ATTACH_HD uint32_t attach_merge_word(uint32_t old_word, uint32_t tail_word, int shared_bits, bool fresh) {
  const uint32_t low = shared_bits > 0 ? (((uint32_t)1 << shared_bits) - 1u) : 0u;
  return ((fresh ? 0xffffffffu : old_word) & low) | (tail_word & ~low);
}

// A remap of dictionary codes (old code -> new code, for a dictionary that grew) keeps the order of the strings: it must be
// strictly increasing and start at or above 0.  -1 = fine, otherwise the first entry that breaks the rule.
inline int64_t attach_remap_check(const int32_t* remap, int64_t n) {
  for (int64_t i = 0; i < n; ++i)
    if (remap[i] < 0 || (i > 0 && remap[i] <= remap[i - 1])) return i;
  return -1;
}

}  // namespace np
