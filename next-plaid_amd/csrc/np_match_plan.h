// np_match_plan.h -- the host side of the text matcher that needs no device: the checks of a packed DFA (np_hip_text_match and
// the NP_F_MATCH leaf refuse a table the device would read out of bounds before any launch), its device image, and the plan
// of DFA groups and string chunks under a byte budget.  Plain C++; tests/cpp/match_plan_check.cpp runs all of it stand-alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../include/nextplaid_hip.h"

namespace np {

// strings per block of the match kernel: 256 lanes, one string each, four ballot words.  Chunks start at multiples of it.
constexpr int64_t NP_MATCH_BLOCK_STRINGS = 256;
constexpr int32_t NP_MATCH_TILE_BYTES = 16384;       // bytes of the text a block stages in LDS at a time
constexpr int32_t NP_MATCH_LDS_TABLE_BYTES = 32768;  // default LDS budget of a table: tile + classes + table = 48.25 KiB,
                                                     // three blocks per CU of 160 KiB
// One lane walks one string, serially, while its block re-stages every tile of it: a string longer than
// NP_MATCH_MAX_STRING_BYTES (include/nextplaid_hip.h) is refused by
// np_hip_index_set_column_text, so that no single dictionary entry can hold a launch for longer than 256 tile iterations of
// one block (the plan's bound on what a long string costs the strings next to it).
static_assert(NP_MATCH_MAX_STRING_BYTES == 256 * (int64_t)NP_MATCH_TILE_BYTES, "the header's bound is 256 tiles");
constexpr int32_t NP_MATCH_LDS_TABLE_MAX = 40960;    // ... and the most np_hip_index_tune("match_lds") gives it (64 KiB a block)

// a device table entry: the next state, and that state's flags where the walk can test them without a second lookup
constexpr uint32_t NP_MATCH_E_STATE = 0x0FFF, NP_MATCH_E_ACCEPT = 0x2000, NP_MATCH_E_DEAD = 0x4000, NP_MATCH_E_MATCHED = 0x8000;

struct MatchDfaInfo {
  int32_t n_states = 0, n_classes = 0, start = 0;
  int64_t image_bytes = 0;   // 256 class bytes + the u16 table, rounded up to 16
};

static inline int64_t match_dfa_words(int64_t n_states, int64_t n_classes) {
  return NP_DFA_HEADER_WORDS + (n_states + 3) / 4 + (n_states * n_classes + 1) / 2;
}

// word i of a packed DFA held as W (u32 at the ABI, i64 inside a filter's values); false: it is not a 32-bit word
template <class W>
static inline bool match_word(const W* w, int64_t i, uint32_t* out) {
  const uint64_t v = (uint64_t)w[i];
  *out = (uint32_t)v;
  return v <= 0xFFFFFFFFull;
}

// One packed DFA (include/nextplaid_hip.h).  0 = well-formed; otherwise NP_ERR_INVALID_ARGUMENT with `why` (at least 160 bytes)
// naming the DFA and the offending state.  Nothing past words[n_words) is read.
template <class W>
inline int match_check_dfa(const W* words, int64_t n_words, int32_t dfa, char* why, size_t why_len, MatchDfaInfo* info) {
  auto fail = [&](int64_t state, const char* what) {
    if (state >= 0)
      snprintf(why, why_len, "DFA %d, state %lld: %s", dfa, (long long)state, what);
    else
      snprintf(why, why_len, "DFA %d: %s", dfa, what);
    return (int)NP_ERR_INVALID_ARGUMENT;
  };
  if (!words) return fail(-1, "NULL words");
  if (n_words < NP_DFA_HEADER_WORDS) return fail(-1, "fewer words than the header");
  uint32_t h[4];
  for (int i = 0; i < 4; ++i)
    if (!match_word(words, i, &h[i])) return fail(-1, "a header word does not fit 32 bits");
  if (h[0] != NP_DFA_MAGIC) return fail(-1, "wrong magic word");
  if (h[1] < 1 || h[1] > NP_DFA_MAX_STATES) return fail(-1, "n_states must be in 1..4096");
  if (h[2] < 1 || h[2] > NP_DFA_MAX_CLASSES) return fail(-1, "n_classes must be in 1..256");
  const int64_t ns = h[1], nc = h[2];
  if (n_words != match_dfa_words(ns, nc)) return fail(-1, "n_words does not match n_states and n_classes");
  if (h[3] >= ns) return fail(-1, "start state out of range");
  for (int b = 0; b < 256; ++b) {
    uint32_t w;
    if (!match_word(words, 4 + b / 4, &w)) return fail(-1, "a class word does not fit 32 bits");
    if (((w >> (8 * (b & 3))) & 0xFF) >= nc) {
      snprintf(why, why_len, "DFA %d: class of byte %d is not below n_classes", dfa, b);
      return (int)NP_ERR_INVALID_ARGUMENT;
    }
  }
  const int64_t f0 = NP_DFA_HEADER_WORDS, t0 = f0 + (ns + 3) / 4;
  for (int64_t s = 0; s < ns; ++s) {
    uint32_t w;
    if (!match_word(words, f0 + s / 4, &w)) return fail(s, "a flag word does not fit 32 bits");
    const uint32_t fl = (w >> (8 * (s & 3))) & 0xFF;
    if (fl & ~(uint32_t)(NP_DFA_ACCEPT_AT_END | NP_DFA_MATCHED | NP_DFA_DEAD)) return fail(s, "unknown flag bits");
    if ((fl & NP_DFA_MATCHED) && !(fl & NP_DFA_ACCEPT_AT_END)) return fail(s, "MATCHED without ACCEPT_AT_END");
    if ((fl & NP_DFA_DEAD) && (fl & NP_DFA_ACCEPT_AT_END)) return fail(s, "DEAD with ACCEPT_AT_END");
    for (int64_t c = 0; c < nc; ++c) {
      const int64_t e = s * nc + c;
      if (!match_word(words, t0 + e / 2, &w)) return fail(s, "a table word does not fit 32 bits");
      const uint32_t to = (w >> (16 * (e & 1))) & 0xFFFF;
      if (to >= ns) return fail(s, "transition to a state that is not below n_states");
      if ((fl & (NP_DFA_MATCHED | NP_DFA_DEAD)) && to != s) return fail(s, "a MATCHED or DEAD state must point to itself");
    }
  }
  if (info) {
    info->n_states = (int32_t)ns;
    info->n_classes = (int32_t)nc;
    info->start = (int32_t)h[3];
    info->image_bytes = (256 + ns * nc * 2 + 15) & ~(int64_t)15;
  }
  return 0;
}

// sizes of a DFA that match_check_dfa has already passed (a filter's programs are checked once, before anything else runs)
template <class W>
inline MatchDfaInfo match_checked_info(const W* words) {
  MatchDfaInfo info;
  info.n_states = (int32_t)words[1];
  info.n_classes = (int32_t)words[2];
  info.start = (int32_t)words[3];
  info.image_bytes = (256 + (int64_t)info.n_states * info.n_classes * 2 + 15) & ~(int64_t)15;
  return info;
}

static inline uint32_t match_entry(uint32_t state, uint32_t flags) {
  return state | ((flags & NP_DFA_ACCEPT_AT_END) ? NP_MATCH_E_ACCEPT : 0u) | ((flags & NP_DFA_DEAD) ? NP_MATCH_E_DEAD : 0u) |
         ((flags & NP_DFA_MATCHED) ? NP_MATCH_E_MATCHED : 0u);
}

// The device image of a CHECKED DFA into image[info.image_bytes]: class_of[256], then the table as u16 entries that carry the
// target's flags (match_entry).  Returns the start state's entry.
template <class W>
inline uint32_t match_build_image(const W* words, const MatchDfaInfo& info, uint8_t* image) {
  const int64_t ns = info.n_states, nc = info.n_classes, f0 = NP_DFA_HEADER_WORDS, t0 = f0 + (ns + 3) / 4;
  memset(image, 0, (size_t)info.image_bytes);
  for (int b = 0; b < 256; ++b) image[b] = (uint8_t)(((uint32_t)words[4 + b / 4] >> (8 * (b & 3))) & 0xFF);
  auto flags = [&](int64_t s) { return ((uint32_t)words[f0 + s / 4] >> (8 * (s & 3))) & 0xFFu; };
  for (int64_t e = 0; e < ns * nc; ++e) {
    const uint32_t to = ((uint32_t)words[t0 + e / 2] >> (16 * (e & 1))) & 0xFFFF;
    const uint16_t v = (uint16_t)match_entry(to, flags(to));
    memcpy(image + 256 + 2 * e, &v, 2);
  }
  return match_entry((uint32_t)info.start, flags(info.start));
}

// Chunks: `dfas` DFAs over `strings` strings at a time (strings a multiple of NP_MATCH_BLOCK_STRINGS unless it is all of them),
// so that per chunk
//     images of the group + dfas * blocks * 32 bytes of verdict bits + 4096  <=  budget.
// All DFAs in one group when their images fit together with one block, otherwise one DFA at a time (the largest image then has
// to fit); false: that does not fit either.  lds[i] = DFA i's table goes to LDS (it fits table_lds_bytes).
struct MatchPlan {
  int32_t dfas = 1;                                  // DFAs per group
  int64_t strings = NP_MATCH_BLOCK_STRINGS;          // strings per chunk
  int32_t tile_bytes = NP_MATCH_TILE_BYTES;
  int32_t table_lds_bytes = NP_MATCH_LDS_TABLE_BYTES;
  int64_t image_bytes = 0;                           // of the largest group
  int64_t blocks() const { return (strings + NP_MATCH_BLOCK_STRINGS - 1) / NP_MATCH_BLOCK_STRINGS; }
  int64_t chunk_words() const { return blocks() * (NP_MATCH_BLOCK_STRINGS / 32); }
  int64_t scratch_bytes() const { return image_bytes + (int64_t)dfas * chunk_words() * 4 + 4096; }
  bool table_in_lds(int64_t image) const { return image - 256 <= table_lds_bytes; }
};
inline bool match_plan(int64_t budget, const int64_t* image_bytes, int32_t n_dfas, int64_t n_strings, int32_t table_lds_bytes,
                       MatchPlan* out) {
  if (n_strings < 1) n_strings = 1;
  int64_t sum = 0, largest = 0;
  for (int32_t i = 0; i < n_dfas; ++i) {
    sum += image_bytes[i];
    if (image_bytes[i] > largest) largest = image_bytes[i];
  }
  if (n_dfas < 1) n_dfas = 1;
  const int64_t all_blocks = (n_strings + NP_MATCH_BLOCK_STRINGS - 1) / NP_MATCH_BLOCK_STRINGS;
  const int64_t block_bytes = NP_MATCH_BLOCK_STRINGS / 8;
  out->table_lds_bytes = table_lds_bytes;
  out->tile_bytes = NP_MATCH_TILE_BYTES;
  if (budget >= sum + 4096 + n_dfas * block_bytes) {
    out->dfas = n_dfas;
    out->image_bytes = sum;
  } else if (budget >= largest + 4096 + block_bytes) {
    out->dfas = 1;
    out->image_bytes = largest;
  } else {
    return false;
  }
  const int64_t b = (budget - out->image_bytes - 4096) / (out->dfas * block_bytes);
  out->strings = b >= all_blocks ? n_strings : b * NP_MATCH_BLOCK_STRINGS;
  return true;
}

}  // namespace np
