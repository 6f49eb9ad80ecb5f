// np_textbuild.hip -- the keyword index built on the device from raw document text (include/nextplaid_hip.h, "Building the
// keyword index on the device"): unicode61 over ASCII, or -- with the caller's table of SQLite's
// classes and folds -- over UTF-8, and trigram.  Stages: classify + count, scan, emit, term numbering, a stable LSD
// radix sort by term id, gather.  Every stage is a sequence of launches: no workgroup waits for another inside a launch,
// nothing a launch writes is read by another workgroup of that launch except a term-table slot (one u32 that goes from
// empty to an instance index once, by atomicCAS, and only ever names bytes of the immutable text), and every position of
// the result comes out of a scan, never out of an atomic counter.
#include <climits>
#include <new>
#include "np_textbuild_dev.h"

namespace np {
namespace {

constexpr uint32_t TB_EMPTY = 0xFFFFFFFFu;
constexpr int TB_NONE = INT_MIN / 2;   // "no token start seen yet"
constexpr int TB_MAX_PROBES = 1024;    // a lane that has not found its term by then reports the table as full

__device__ __forceinline__ uint32_t tb_fold(uint32_t c) { return (c - 'A' < 26u) ? c + 32u : c; }
__device__ __forceinline__ bool tb_tok(uint32_t c) { return (c - '0' < 10u) || ((c | 0x20u) - 'a' < 26u); }

__device__ __forceinline__ int tb_wave_incl_max(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d);
    if (lane >= d) v = max(v, o);
  }
  return v;
}

__device__ __forceinline__ uint32_t tb_wave_incl_sum(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

__device__ __forceinline__ uint32_t tb_byte(const uint32_t* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu; }

// ---- unicode61: one wave per document, 16 bytes per lane and step -------------------------------------------------------
// The wave walks the 16-byte lines that hold the document (bytes of a line outside the document count as separators), a
// tile of tile_lanes lines per step.  A token ends where a separator follows a token character, and its start is the most
// recent start before that: both survive a lane and a tile edge as a carried bit and a carried position.  The k-th end of a
// document is its k-th token.  EMIT = false: the fallback verdict and the token count; EMIT = true: the instances, at the
// places the scan of the counts gave them.
template <bool EMIT>
__global__ __launch_bounds__(256) void tb_walk_unicode(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                        int64_t n_docs, int tile_lanes, int max_tok, uint32_t* count,
                                                        uint32_t* fb, const int64_t* __restrict__ first, uint32_t* i_doc,
                                                        uint32_t* i_rel, uint32_t* i_len) {
  const int lane = threadIdx.x & 63;
  const int64_t doc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (doc >= n_docs) return;   // wave-uniform, as every exit and trip count below
  const int64_t b = offs[doc], e = offs[doc + 1];
  if (EMIT) {
    if (fb[doc] || count[doc] == 0) return;
  } else if (b == e) {
    if (lane == 0) count[doc] = 0, fb[doc] = 0;
    return;
  }
  const int64_t base = EMIT ? first[doc] : 0;
  const int64_t len = e - b;
  const int64_t r0 = (b & ~(int64_t)15) - b;   // -15..0: the first loaded byte, relative to the document
  int open = TB_NONE;                          // the most recent token start before this tile
  uint32_t carry = 0, ntok = 0;                // was the last byte of the previous tile a token character; tokens ended so far
  bool bad = false;
  for (int64_t rt = r0; rt <= len; rt += (int64_t)tile_lanes * 16) {   // position len is walked: a token may end there
    const int64_t r = rt + lane * 16;
    uint32_t m = 0;
    if (lane < tile_lanes && r <= len) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b + r);   // at most 15 bytes past the text: it is padded
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t c = tb_byte(w, k);
        if (r + k >= 0 && r + k < len) {
          bad |= (c & 0x80u) != 0;
          m |= tb_tok(c) ? (1u << k) : 0u;
        }
      }
    }
    const uint32_t pm = __shfl_up(m, 1);
    const uint32_t prevc = lane == 0 ? carry : (lane < tile_lanes ? (pm >> 15) & 1u : 0u);
    const uint32_t sh = ((m << 1) | prevc) & 0xFFFFu;   // bit k: the byte before k is a token character
    const uint32_t s = m & ~sh, f = ~m & sh;            // starts; ends (exclusive)
    const int ls = s ? (int)r + (31 - __clz(s)) : TB_NONE;
    const int inc = tb_wave_incl_max(ls, lane);
    int exc = __shfl_up(inc, 1);
    exc = lane == 0 ? open : max(exc, open);
    const uint32_t nf = __popc(f);
    const uint32_t incf = tb_wave_incl_sum(nf, lane);
    uint32_t k = ntok + incf - nf;
    for (uint32_t ff = f; ff; ff &= ff - 1, ++k) {
      const int j = __ffs(ff) - 1;
      const uint32_t sj = s & ((1u << j) - 1u);
      const int st = sj ? (int)r + (31 - __clz(sj)) : exc;
      const int tl = (int)r + j - st;
      bad |= tl > max_tok;
      if (EMIT) {
        const int64_t n = base + k;
        i_doc[n] = (uint32_t)doc;
        i_rel[n] = (uint32_t)st;
        i_len[n] = (uint32_t)tl;
      }
    }
    ntok += __shfl(incf, 63);
    open = max(open, __shfl(inc, 63));
    carry = (__shfl(m, tile_lanes - 1) >> 15) & 1u;
    if (!EMIT && __any(bad)) break;
  }
  if (!EMIT) {
    const bool fall = __any(bad);
    if (lane == 0) count[doc] = fall ? 0u : ntok, fb[doc] = fall ? 1u : 0u;
  }
}

// ---- unicode61 over UTF-8: the same walk, a class per code point out of the caller's table ------------------------------
// Every byte takes the class of the code point it belongs to.  A lane decodes the sequences whose lead byte lies in its
// line -- out of a window of 20 bytes, the line and the four behind it, so a sequence may run into the next lane's line or
// the next tile -- and hands the up to three bits that leave its line to the next lane.  A mark takes the token bit of the
// byte before it: inside a lane one carry-propagating add resolves every run of marks, and a lane's last bit is 0, 1 or, for
// a lane of marks alone, "what came in", so one scan of {0, 1, pass} over the lanes and one carried bit per tile give every
// lane its incoming bit.  Starts and ends then come out of tb_walk_unicode's mask arithmetic; a token's length is its raw
// bytes, marks included.  Bytes below 0x80 take the ASCII rule without a table read (the host checked entries 0..127).
constexpr uint32_t TB_PASS = 2u;

// bit k of the result: byte k is a token byte -- tok | the marks that a token bit (or `in`, before bit 0) runs into
__device__ __forceinline__ uint32_t tb_resolve_marks(uint32_t tok, uint32_t mark, uint32_t in) {
  const uint32_t hit = ((tok << 1) | in) & mark;   // the first mark of every run that continues a token
  return tok | (mark & ~(mark + hit));             // the add carries through exactly those runs
}

template <bool EMIT>
__global__ __launch_bounds__(256) void tb_walk_utf8(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                     int64_t n_docs, int tile_lanes, int max_tok,
                                                     const uint32_t* __restrict__ utab, uint32_t utab_len, uint32_t* count,
                                                     uint32_t* fb, const int64_t* __restrict__ first, uint32_t* i_doc,
                                                     uint32_t* i_rel, uint32_t* i_len) {
  const int lane = threadIdx.x & 63;
  const int64_t doc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (doc >= n_docs) return;   // wave-uniform, as every exit and trip count below
  const int64_t b = offs[doc], e = offs[doc + 1];
  if (EMIT) {
    if (fb[doc] || count[doc] == 0) return;
  } else if (b == e) {
    if (lane == 0) count[doc] = 0, fb[doc] = 0;
    return;
  }
  const int64_t base = EMIT ? first[doc] : 0;
  const int64_t len = e - b;
  const int64_t r0 = (b & ~(int64_t)15) - b;
  int open = TB_NONE;
  uint32_t carry = 0, ntok = 0;   // the token bit of the previous tile's last byte; tokens ended so far
  uint32_t carry_spill = 0;       // what the previous tile's last lane hands on: token, mark and covered bits, 4 each
  bool bad = false;
  for (int64_t rt = r0; rt <= len; rt += (int64_t)tile_lanes * 16) {
    const int64_t r = rt + lane * 16;
    uint32_t tok = 0, mark = 0, cover = 0, cont = 0;   // 20 bits each: bit k is byte r + k; cover = bytes behind a lead
    if (lane < tile_lanes && r <= len) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b + r);   // at most 19 bytes past the text: it is padded
      const uint32_t w[5] = {v.x, v.y, v.z, v.w, *reinterpret_cast<const uint32_t*>(text + b + r + 16)};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t c = tb_byte(w, k);
        if (r + k < 0 || r + k >= len) continue;
        if (c < 0x80u) {
          tok |= tb_tok(c) ? (1u << k) : 0u;
        } else if (c < 0xC0u) {
          cont |= 1u << k;
        } else {
          const uint32_t c1 = tb_byte(w, k + 1), c2 = tb_byte(w, k + 2), c3 = tb_byte(w, k + 3);
          const int n = c < 0xE0u ? 2 : c < 0xF0u ? 3 : 4;
          bool ok = (c1 & 0xC0u) == 0x80u && r + k + n <= len;   // the next document's bytes never complete a sequence
          uint32_t cp;
          if (n == 2) {
            cp = ((c & 0x1Fu) << 6) | (c1 & 0x3Fu);
            ok = ok && cp >= 0x80u;
          } else if (n == 3) {
            cp = ((c & 0x0Fu) << 12) | ((c1 & 0x3Fu) << 6) | (c2 & 0x3Fu);
            ok = ok && (c2 & 0xC0u) == 0x80u && cp >= 0x800u && cp - 0xD800u >= 0x800u;
          } else {
            cp = ((c & 0x07u) << 18) | ((c1 & 0x3Fu) << 12) | ((c2 & 0x3Fu) << 6) | (c3 & 0x3Fu);
            ok = ok && c < 0xF8u && (c2 & 0xC0u) == 0x80u && (c3 & 0xC0u) == 0x80u && cp - 0x10000u < 0x100000u;
          }
          ok = ok && cp < utab_len;
          if (ok) {
            const uint32_t cls = utab[cp] >> 30, bits = ((1u << n) - 1u) << k;
            tok |= cls == 1u ? bits : 0u;
            mark |= cls == 2u ? bits : 0u;
            cover |= bits & ~(1u << k);
          } else {
            bad = true;
          }
        }
      }
    }
    const uint32_t spill = (tok >> 16) | ((mark >> 16) << 4) | ((cover >> 16) << 8);
    const uint32_t ps = __shfl_up(spill, 1);
    const uint32_t from = lane == 0 ? carry_spill : (lane < tile_lanes ? ps : 0u);
    tok = (tok & 0xFFFFu) | (from & 15u);
    mark = (mark & 0xFFFFu) | ((from >> 4) & 15u);
    cover = (cover & 0xFFFFu) | ((from >> 8) & 15u);
    bad |= (cont & ~cover) != 0;   // a continuation byte that no lead covers
    // the token bit behind this lane's line as a function of the one before it: 0, 1 or pass
    uint32_t out = mark == 0xFFFFu ? TB_PASS : (tb_resolve_marks(tok, mark, 0u) >> 15) & 1u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(out, d);
      if (lane >= d && out == TB_PASS) out = o;
    }
    const uint32_t po = __shfl_up(out, 1);
    const uint32_t prevc = lane == 0 ? carry : (lane < tile_lanes ? (po == TB_PASS ? carry : po) : 0u);
    const uint32_t m = tb_resolve_marks(tok, mark, prevc) & 0xFFFFu;
    const uint32_t sh = ((m << 1) | prevc) & 0xFFFFu;
    const uint32_t s = m & ~sh, f = ~m & sh;
    const int ls = s ? (int)r + (31 - __clz(s)) : TB_NONE;
    const int inc = tb_wave_incl_max(ls, lane);
    int exc = __shfl_up(inc, 1);
    exc = lane == 0 ? open : max(exc, open);
    const uint32_t nf = __popc(f);
    const uint32_t incf = tb_wave_incl_sum(nf, lane);
    uint32_t k = ntok + incf - nf;
    for (uint32_t ff = f; ff; ff &= ff - 1, ++k) {
      const int j = __ffs(ff) - 1;
      const uint32_t sj = s & ((1u << j) - 1u);
      const int st = sj ? (int)r + (31 - __clz(sj)) : exc;
      const int tl = (int)r + j - st;
      bad |= tl > max_tok;
      if (EMIT) {
        const int64_t n = base + k;
        i_doc[n] = (uint32_t)doc;
        i_rel[n] = (uint32_t)st;
        i_len[n] = (uint32_t)tl;
      }
    }
    ntok += __shfl(incf, 63);
    open = max(open, __shfl(inc, 63));
    carry = (__shfl(m, tile_lanes - 1) >> 15) & 1u;
    carry_spill = __shfl(spill, tile_lanes - 1);
    if (!EMIT && __any(bad)) break;
  }
  if (!EMIT) {
    const bool fall = __any(bad);
    if (lane == 0) count[doc] = fall ? 0u : ntok, fb[doc] = fall ? 1u : 0u;
  }
}

// ---- trigram ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tb_classify_trigram(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                            int64_t n_docs, int tile_lanes, uint32_t* count, uint32_t* fb) {
  const int lane = threadIdx.x & 63;
  const int64_t doc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (doc >= n_docs) return;
  const int64_t b = offs[doc], e = offs[doc + 1];
  const int64_t len = e - b;
  const int64_t r0 = (b & ~(int64_t)15) - b;
  bool bad = false;
  for (int64_t rt = r0; rt < len; rt += (int64_t)tile_lanes * 16) {
    const int64_t r = rt + lane * 16;
    if (lane < tile_lanes && r < len) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b + r);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t c = tb_byte(w, k);
        if (r + k >= 0 && r + k < len) bad |= c == 0u || (c & 0x80u) != 0;
      }
    }
    if (__any(bad)) break;
  }
  const bool fall = __any(bad);
  if (lane == 0) count[doc] = fall || len < 3 ? 0u : (uint32_t)(len - 2), fb[doc] = fall ? 1u : 0u;
}

// instance first[doc] + i = the three folded bytes at offset i: its 21-bit key, and the key's bit in the presence bitmap
__global__ __launch_bounds__(256) void tb_emit_trigram(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                        int64_t n_docs, int tile_lanes, const uint32_t* __restrict__ count,
                                                        const int64_t* __restrict__ first, uint32_t* i_doc, uint32_t* i_rel,
                                                        uint32_t* key, uint32_t* bitmap) {
  const int lane = threadIdx.x & 63;
  const int64_t doc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (doc >= n_docs) return;
  if (count[doc] == 0) return;
  const int64_t b = offs[doc], e = offs[doc + 1];
  const int64_t len = e - b, base = first[doc];
  const int64_t r0 = (b & ~(int64_t)15) - b;
  for (int64_t rt = r0; rt <= len - 3; rt += (int64_t)tile_lanes * 16) {
    const int64_t r = rt + lane * 16;
    if (lane < tile_lanes && r <= len - 3) {
      const uint4 v = *reinterpret_cast<const uint4*>(text + b + r);
      const uint32_t w[5] = {v.x, v.y, v.z, v.w, *reinterpret_cast<const uint32_t*>(text + b + r + 16)};   // inside the padding
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        if (r + k >= 0 && r + k <= len - 3) {
          const uint32_t kk = (tb_fold(tb_byte(w, k)) << 14) | (tb_fold(tb_byte(w, k + 1)) << 7) | tb_fold(tb_byte(w, k + 2));
          const int64_t n = base + r + k;
          i_doc[n] = (uint32_t)doc;
          i_rel[n] = (uint32_t)(r + k);
          key[n] = kk;
          atomicOr(&bitmap[kk >> 5], 1u << (kk & 31u));
        }
      }
    }
  }
}

__global__ void tb_popc(const uint32_t* __restrict__ bitmap, int64_t n, uint32_t* cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) cnt[i] = __popc(bitmap[i]);
}

// key -> its rank among the keys present; val = the instance's own index
__global__ void tb_assign_trigram(uint32_t* key, uint32_t* val, int64_t n, const uint32_t* __restrict__ bitmap,
                                  const uint32_t* __restrict__ prefix) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key[i];
  key[i] = prefix[k >> 5] + __popc(bitmap[k >> 5] & ((1u << (k & 31u)) - 1u));
  val[i] = (uint32_t)i;
}

// ---- unicode61: the term table -------------------------------------------------------------------------------------------
// A slot holds the index of the instance that claimed it.  A lane whose slot is taken compares its token with that
// instance's, byte for byte after folding: both lie in the text and in the instance arrays of the launch before, so what a
// lane reads of this launch's writes is the slot word alone.  Equal terms walk the same probe sequence and slots are never
// released, so a term owns exactly one slot whatever the arrival order; which of its instances sits there does not matter.
__global__ __launch_bounds__(256) void tb_insert(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                  const uint32_t* __restrict__ i_doc, const uint32_t* __restrict__ i_rel,
                                                  const uint32_t* __restrict__ i_len, int64_t n_inst, uint32_t* tab, uint32_t mask,
                                                  uint32_t* slot_of, uint32_t* overflow) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_inst) return;
  const uint8_t* p = text + offs[i_doc[n]] + i_rel[n];
  const uint32_t len = i_len[n];
  uint32_t h = 2166136261u;
  for (uint32_t i = 0; i < len; ++i) h = (h ^ tb_fold(p[i])) * 16777619u;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  uint32_t slot = h & mask;
  const uint32_t probes = mask < (uint32_t)TB_MAX_PROBES ? mask + 1u : (uint32_t)TB_MAX_PROBES;
  for (uint32_t t = 0; t < probes; ++t, slot = (slot + 1u) & mask) {
    uint32_t old = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // spares a claimed slot the CAS
    if (old == TB_EMPTY) old = atomicCAS(&tab[slot], TB_EMPTY, (uint32_t)n);
    if (old == TB_EMPTY) {
      slot_of[n] = slot;
      return;
    }
    if (i_len[old] == len) {
      const uint8_t* q = text + offs[i_doc[old]] + i_rel[old];
      uint32_t i = 0;
      while (i < len && tb_fold(p[i]) == tb_fold(q[i])) ++i;
      if (i == len) {
        slot_of[n] = slot;
        return;
      }
    }
  }
  slot_of[n] = TB_EMPTY;
  atomicAdd(overflow, 1u);
}

// The next folded code point of the token p[0, len) from byte i on, marks skipped; TB_EMPTY behind the last.  The token
// passed the walk: its sequences are well formed and inside the table, and each is a token character or a mark.
__device__ __forceinline__ uint32_t tb_next_folded(const uint8_t* p, uint32_t& i, uint32_t len, const uint32_t* __restrict__ utab) {
  while (i < len) {
    const uint32_t c = p[i];
    if (c < 0x80u) {
      ++i;
      return tb_fold(c);
    }
    uint32_t cp;
    if (c < 0xE0u) cp = ((c & 0x1Fu) << 6) | (p[i + 1] & 0x3Fu), i += 2;
    else if (c < 0xF0u) cp = ((c & 0x0Fu) << 12) | ((p[i + 1] & 0x3Fu) << 6) | (p[i + 2] & 0x3Fu), i += 3;
    else cp = ((c & 0x07u) << 18) | ((p[i + 1] & 0x3Fu) << 12) | ((p[i + 2] & 0x3Fu) << 6) | (p[i + 3] & 0x3Fu), i += 4;
    const uint32_t e = utab[cp];
    if ((e >> 30) == 1u) return e & 0x1FFFFFu;
  }
  return TB_EMPTY;
}

// tb_insert over folded code points: two instances of different raw lengths may be one term (a precomposed letter, the
// plain one, the plain one and a mark), so a taken slot is compared stream against stream, never by length first.
__global__ __launch_bounds__(256) void tb_insert_utf8(const uint8_t* __restrict__ text, const int64_t* __restrict__ offs,
                                                       const uint32_t* __restrict__ i_doc, const uint32_t* __restrict__ i_rel,
                                                       const uint32_t* __restrict__ i_len, int64_t n_inst,
                                                       const uint32_t* __restrict__ utab, uint32_t* tab, uint32_t mask,
                                                       uint32_t* slot_of, uint32_t* overflow) {
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= n_inst) return;
  const uint8_t* p = text + offs[i_doc[n]] + i_rel[n];
  const uint32_t len = i_len[n];
  uint32_t h = 2166136261u;
  for (uint32_t i = 0;;) {
    const uint32_t cp = tb_next_folded(p, i, len, utab);
    if (cp == TB_EMPTY) break;
    h = (h ^ cp) * 16777619u;
  }
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  uint32_t slot = h & mask;
  const uint32_t probes = mask < (uint32_t)TB_MAX_PROBES ? mask + 1u : (uint32_t)TB_MAX_PROBES;
  for (uint32_t t = 0; t < probes; ++t, slot = (slot + 1u) & mask) {
    uint32_t old = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == TB_EMPTY) old = atomicCAS(&tab[slot], TB_EMPTY, (uint32_t)n);
    if (old == TB_EMPTY) {
      slot_of[n] = slot;
      return;
    }
    const uint8_t* q = text + offs[i_doc[old]] + i_rel[old];
    const uint32_t qlen = i_len[old];
    uint32_t i = 0, j = 0, a, c;
    do {
      a = tb_next_folded(p, i, len, utab);
      c = tb_next_folded(q, j, qlen, utab);
    } while (a == c && a != TB_EMPTY);
    if (a == c) {
      slot_of[n] = slot;
      return;
    }
  }
  slot_of[n] = TB_EMPTY;
  atomicAdd(overflow, 1u);
}

__global__ void tb_flags(const uint32_t* __restrict__ tab, int64_t slots, uint32_t* flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < slots) flags[i] = tab[i] != TB_EMPTY ? 1u : 0u;
}

// occupied slot -> its place c in the compacted list and where its term's bytes are
__global__ void tb_compact(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ slot_c, int64_t slots,
                           const uint32_t* __restrict__ i_doc, const uint32_t* __restrict__ i_rel,
                           const uint32_t* __restrict__ i_len, uint32_t* rep_doc, uint32_t* rep_rel, uint32_t* rep_len) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots) return;
  const uint32_t rep = tab[i];
  if (rep == TB_EMPTY) return;
  const uint32_t c = slot_c[i];
  rep_doc[c] = i_doc[rep];
  rep_rel[c] = i_rel[rep];
  rep_len[c] = i_len[rep];
}

// key: the instance's slot -> its term id; val = the instance's own index
__global__ void tb_assign_unicode(uint32_t* key, uint32_t* val, int64_t n, const uint32_t* __restrict__ slot_c,
                                  const uint32_t* __restrict__ rank) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  key[i] = rank[slot_c[key[i]]];
  val[i] = (uint32_t)i;
}

// ---- the radix pass: one wave per block of NP_TB_SORT_CHUNK keys ----------------------------------------------------------
__global__ __launch_bounds__(64) void tb_radix_hist(const uint32_t* __restrict__ keys, int64_t n, int shift, uint32_t* hist,
                                                     int64_t nblk) {
  __shared__ uint32_t h[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) h[d] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * NP_TB_SORT_CHUNK;
  for (int r = 0; r < NP_TB_SORT_CHUNK / 256; ++r) {
    const int64_t i = base + ((int64_t)r * 64 + lane) * 4;
    if (i + 3 < n) {
      const uint4 v = *reinterpret_cast<const uint4*>(keys + i);
      atomicAdd(&h[(v.x >> shift) & 255u], 1u);
      atomicAdd(&h[(v.y >> shift) & 255u], 1u);
      atomicAdd(&h[(v.z >> shift) & 255u], 1u);
      atomicAdd(&h[(v.w >> shift) & 255u], 1u);
    } else {
      for (int64_t j = i; j < n && j < i + 4; ++j) atomicAdd(&h[(keys[j] >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  for (int d = lane; d < 256; d += 64) hist[(int64_t)d * nblk + blockIdx.x] = h[d];
}

// Stable: a block's keys go out in rounds of 64 in input order; inside a round a key's place among the keys of its digit is
// the number of lower lanes with that digit (eight ballots), and the digit's running base moves on by the round's count.
__global__ __launch_bounds__(64) void tb_radix_scatter(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        uint32_t* keys_out, uint32_t* vals_out, int64_t n, int shift,
                                                        const uint32_t* __restrict__ hist, int64_t nblk) {
  __shared__ uint32_t base[256];
  const int lane = threadIdx.x;
  for (int d = lane; d < 256; d += 64) base[d] = hist[(int64_t)d * nblk + blockIdx.x];
  __syncthreads();
  const int64_t b0 = (int64_t)blockIdx.x * NP_TB_SORT_CHUNK;
  for (int r = 0; r < NP_TB_SORT_CHUNK / 64; ++r) {
    const int64_t i = b0 + (int64_t)r * 64 + lane;
    if (b0 + (int64_t)r * 64 >= n) break;   // wave-uniform
    const bool act = i < n;
    const uint32_t k = act ? keys[i] : 0u, v = act ? vals[i] : 0u;
    const uint32_t d = (k >> shift) & 255u;
    unsigned long long peers = __ballot(act);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long bm = __ballot(on);
      peers &= on ? bm : ~bm;
    }
    const uint32_t rank = __popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t dst = act ? base[d] + rank : 0u;
    __syncthreads();
    if (act && rank == 0) base[d] += __popcll(peers);
    __syncthreads();
    if (act) {
      keys_out[dst] = k;
      vals_out[dst] = v;
    }
  }
}

__global__ void tb_gather(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals, int64_t n, int64_t n_terms,
                          const uint32_t* __restrict__ i_doc, const uint32_t* __restrict__ i_rel,
                          const int64_t* __restrict__ first, int unicode, int64_t* inst_doc, int32_t* inst_pos, int64_t* toff) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t v = vals[i], d = i_doc[v];
  inst_doc[i] = (int64_t)d;
  inst_pos[i] = unicode ? (int32_t)((int64_t)v - first[d]) : (int32_t)i_rel[v];
  const uint32_t k = keys[i];
  if (i == 0 || keys[i - 1] != k) toff[k] = i;   // every term has an instance: every entry is written
  if (i == n - 1) toff[n_terms] = n;
}

}  // namespace
}  // namespace np

using namespace np;

namespace np {
namespace {

// the device arrays of one call, and the bytes they hold against the workspace
struct TbWork {
  int64_t held = 0, limit = 0;
  template <class T>
  int take(DevPtr<T>& p, int64_t n, const char* what) {
    const int64_t bytes = textbuild_up256(std::max<int64_t>(n, 1) * (int64_t)sizeof(T));
    if (limit > 0 && held + bytes > limit) {
      set_error("np_hip_text_build: the workspace of %lld bytes does not hold the call: %lld held, %lld more for %s (a "
                "whole-corpus sort: build in document ranges and merge them, np_hip_text_build_merge)",
                (long long)limit, (long long)held, (long long)bytes, what);
      return NP_ERR_OUT_OF_MEMORY;
    }
    NP_TRY(p.alloc((size_t)(bytes / (int64_t)sizeof(T))));
    held += bytes;
    return NP_OK;
  }
};

int text_build_impl(int device, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const TextBuildPlan& plan,
                    np_text_build* B, np_text_build_report* rep) {
  const auto t_all = Clock::now();
  const bool unicode = plan.tokenizer == NP_TOK_UNICODE61;
  const bool utf8 = unicode && plan.unicode_table != nullptr;
  const int64_t utab_len = utf8 ? plan.unicode_table_len : 0;
  const int64_t N = plan.text_bytes;
  const int tile_lanes = plan.tile_bytes / 16;
  char why[256];
  if (!unicode && textbuild_check_instances(textbuild_trigram_upper(offsets, n_docs), why, sizeof(why)) != NP_OK) {
    set_error("%s", why);
    return NP_ERR_SHAPE;
  }
  NP_TRY(build_check_device(device));
  DeviceGuard g(device);
  TbWork W;
  {
    size_t free_b = 0, total_b = 0;
    NP_HIP(hipMemGetInfo(&free_b, &total_b));
    W.limit = plan.workspace_bytes > 0 ? plan.workspace_bytes : (int64_t)(free_b - free_b / 16);
  }
  if (textbuild_bytes_docs(N, n_docs, utab_len) > W.limit) {
    set_error("np_hip_text_build: the workspace of %lld bytes does not hold the text and the per-document arrays (%lld bytes; a "
              "whole-corpus sort: build in document ranges and merge them, np_hip_text_build_merge)",
              (long long)W.limit, (long long)textbuild_bytes_docs(N, n_docs, utab_len));
    return NP_ERR_OUT_OF_MEMORY;
  }
  TbStream S;
  NP_HIP(hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking));
  hipStream_t st = S.st;
  B->device = device;
  B->tokenizer = plan.tokenizer;
  B->n_docs = n_docs;

  // ---- upload
  auto t0 = Clock::now();
  DevPtr<uint8_t> d_text;
  DevPtr<int64_t> d_offs, d_first;
  DevPtr<uint32_t> d_count, d_fb, d_utab;
  DevPtr<uint64_t> d_sums;
  int64_t sums_cap = 0;
  auto need_sums = [&](int64_t n) -> int {
    const int64_t want = textbuild_scan_sums(n);
    if (want <= sums_cap) return NP_OK;
    NP_HIP(hipStreamSynchronize(st));
    W.held -= sums_cap ? textbuild_up256(sums_cap * 8) : 0;
    sums_cap = want;
    return W.take(d_sums, want, "the scan's block sums");
  };
  NP_TRY(W.take(d_text, N + NP_TB_TEXT_PAD, "the text"));
  NP_TRY(W.take(d_offs, n_docs + 1, "the offsets"));
  NP_TRY(W.take(d_first, n_docs + 1, "the documents' first instances"));
  NP_TRY(W.take(d_count, n_docs + 1, "the documents' token counts"));
  NP_TRY(W.take(d_fb, n_docs + 1, "the fallback flags"));
  NP_TRY(need_sums(n_docs + 1));
  if (utf8) {
    NP_TRY(W.take(d_utab, utab_len, "the unicode61 table"));
    NP_HIP(hipMemcpyAsync(d_utab.get(), plan.unicode_table, (size_t)utab_len * 4, hipMemcpyHostToDevice, st));
  }
  if (N > 0) NP_HIP(hipMemcpyAsync(d_text.get(), bytes, (size_t)N, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemsetAsync(d_text.get() + N, 0, (size_t)NP_TB_TEXT_PAD, st));
  NP_HIP(hipMemcpyAsync(d_offs.get(), offsets, (size_t)(n_docs + 1) * 8, hipMemcpyHostToDevice, st));
  NP_HIP(hipStreamSynchronize(st));
  const double ms_upload = ms_since(t0);

  // ---- classify, count, scan
  t0 = Clock::now();
  const unsigned doc_grid = grid_of(n_docs, 4);
  if (n_docs > 0) {
    if (utf8)
      hipLaunchKernelGGL(tb_walk_utf8<false>, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                         (const int64_t*)d_offs.get(), n_docs, tile_lanes, plan.max_token, (const uint32_t*)d_utab.get(),
                         (uint32_t)utab_len, d_count.get(), d_fb.get(), (const int64_t*)nullptr, (uint32_t*)nullptr,
                         (uint32_t*)nullptr, (uint32_t*)nullptr);
    else if (unicode)
      hipLaunchKernelGGL(tb_walk_unicode<false>, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                         (const int64_t*)d_offs.get(), n_docs, tile_lanes, plan.max_token, d_count.get(), d_fb.get(),
                         (const int64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
    else
      hipLaunchKernelGGL(tb_classify_trigram, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                         (const int64_t*)d_offs.get(), n_docs, tile_lanes, d_count.get(), d_fb.get());
    NP_HIP(hipGetLastError());
  }
  NP_TRY(tb_scan<int64_t>(st, d_count.get(), n_docs, d_first.get(), d_sums.get()));
  int64_t n_inst = 0;
  std::vector<uint32_t> h_fb((size_t)n_docs);
  NP_HIP(hipMemcpyAsync(&n_inst, d_first.get() + n_docs, 8, hipMemcpyDeviceToHost, st));
  if (n_docs > 0) NP_HIP(hipMemcpyAsync(h_fb.data(), d_fb.get(), (size_t)n_docs * 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipStreamSynchronize(st));
  B->fallback.clear();
  for (int64_t i = 0; i < n_docs; ++i)
    if (h_fb[(size_t)i]) B->fallback.push_back(i);
  const double ms_classify = ms_since(t0);
  if (textbuild_check_instances(n_inst, why, sizeof(why)) != NP_OK) {
    set_error("%s", why);
    return NP_ERR_SHAPE;
  }
  int32_t bits = unicode ? textbuild_hash_bits(n_inst, plan.hash_bits_forced) : 0;
  {
    const int64_t need = textbuild_bytes_total(N, n_docs, n_inst, plan.tokenizer, bits, utab_len);
    if (need > W.limit) {
      set_error("np_hip_text_build: the workspace of %lld bytes does not hold the call: %lld instances need %lld bytes (a "
                "whole-corpus sort: build in document ranges and merge them, np_hip_text_build_merge)",
                (long long)W.limit, (long long)n_inst, (long long)need);
      return NP_ERR_OUT_OF_MEMORY;
    }
  }
  B->n_inst = n_inst;
  double ms_emit = 0, ms_terms = 0, ms_sort = 0;
  int32_t retries = 0, passes = 0;
  int64_t n_terms = 0;
  B->term_bytes.clear();
  B->term_byte_offsets.assign(1, 0);

  if (n_inst == 0) {
    NP_TRY(W.take(B->d_toff, 1, "term_offsets"));
    NP_HIP(hipMemsetAsync(B->d_toff.get(), 0, 8, st));
    NP_HIP(hipStreamSynchronize(st));
    bits = 0;
  } else {
    // ---- emit
    t0 = Clock::now();
    DevPtr<uint32_t> i_doc, i_rel, i_len, key_a, key_b, val_a, val_b, d_bitmap;
    NP_TRY(W.take(i_doc, n_inst, "the instances' documents"));
    NP_TRY(W.take(i_rel, n_inst, "the instances' offsets"));
    NP_TRY(W.take(key_a, n_inst, "the sort keys"));
    NP_TRY(W.take(val_a, n_inst, "the sort values"));
    NP_TRY(W.take(key_b, n_inst, "the sort keys"));
    NP_TRY(W.take(val_b, n_inst, "the sort values"));
    const int64_t bm_words = NP_TB_TRIGRAM_KEYS / 32;
    if (unicode) {
      NP_TRY(W.take(i_len, n_inst, "the instances' lengths"));
      if (utf8)
        hipLaunchKernelGGL(tb_walk_utf8<true>, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                           (const int64_t*)d_offs.get(), n_docs, tile_lanes, plan.max_token, (const uint32_t*)d_utab.get(),
                           (uint32_t)utab_len, d_count.get(), d_fb.get(), (const int64_t*)d_first.get(), i_doc.get(), i_rel.get(),
                           i_len.get());
      else
        hipLaunchKernelGGL(tb_walk_unicode<true>, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                         (const int64_t*)d_offs.get(), n_docs, tile_lanes, plan.max_token, d_count.get(), d_fb.get(),
                         (const int64_t*)d_first.get(), i_doc.get(), i_rel.get(), i_len.get());
    } else {
      NP_TRY(W.take(d_bitmap, bm_words, "the trigram bitmap"));
      NP_HIP(hipMemsetAsync(d_bitmap.get(), 0, (size_t)bm_words * 4, st));
      hipLaunchKernelGGL(tb_emit_trigram, dim3(doc_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                         (const int64_t*)d_offs.get(), n_docs, tile_lanes, (const uint32_t*)d_count.get(),
                         (const int64_t*)d_first.get(), i_doc.get(), i_rel.get(), key_a.get(), d_bitmap.get());
    }
    NP_HIP(hipGetLastError());
    NP_HIP(hipStreamSynchronize(st));
    ms_emit = ms_since(t0);

    // ---- term ids into key_a, instance indexes into val_a
    t0 = Clock::now();
    const unsigned inst_grid = grid_of(n_inst, 256);
    if (unicode) {
      DevPtr<uint32_t> d_tab, d_flags, d_slot_c, d_ovf, rep_doc, rep_rel, rep_len, d_rank;
      NP_TRY(W.take(d_ovf, 1, "the overflow count"));
      int64_t slots = 0;
      for (;;) {
        slots = (int64_t)1 << bits;
        const int64_t before = W.held;
        NP_TRY(W.take(d_tab, slots, "the term table"));
        NP_HIP(hipMemsetAsync(d_tab.get(), 0xFF, (size_t)slots * 4, st));
        NP_HIP(hipMemsetAsync(d_ovf.get(), 0, 4, st));
        if (utf8)
          hipLaunchKernelGGL(tb_insert_utf8, dim3(inst_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(),
                             (const int64_t*)d_offs.get(), (const uint32_t*)i_doc.get(), (const uint32_t*)i_rel.get(),
                             (const uint32_t*)i_len.get(), n_inst, (const uint32_t*)d_utab.get(), d_tab.get(), (uint32_t)(slots - 1),
                             key_a.get(), d_ovf.get());
        else
          hipLaunchKernelGGL(tb_insert, dim3(inst_grid), dim3(256), 0, st, (const uint8_t*)d_text.get(), (const int64_t*)d_offs.get(),
                             (const uint32_t*)i_doc.get(), (const uint32_t*)i_rel.get(), (const uint32_t*)i_len.get(), n_inst,
                             d_tab.get(), (uint32_t)(slots - 1), key_a.get(), d_ovf.get());
        NP_HIP(hipGetLastError());
        uint32_t ovf = 0;
        NP_HIP(hipMemcpyAsync(&ovf, d_ovf.get(), 4, hipMemcpyDeviceToHost, st));
        NP_HIP(hipStreamSynchronize(st));
        if (ovf == 0) break;
        if (bits >= NP_TB_HASH_BITS_MAX) {
          set_error("np_hip_text_build: the term table is full at 2^%d slots", bits);
          return NP_ERR_OUT_OF_MEMORY;
        }
        d_tab.reset();
        W.held = before;
        ++bits;
        ++retries;
      }
      NP_TRY(W.take(d_flags, slots, "the table's flags"));
      NP_TRY(W.take(d_slot_c, slots + 1, "the slots' places"));
      NP_TRY(need_sums(slots + 1));
      hipLaunchKernelGGL(tb_flags, dim3(grid_of(slots, 256)), dim3(256), 0, st, (const uint32_t*)d_tab.get(), slots, d_flags.get());
      NP_TRY(tb_scan<uint32_t>(st, d_flags.get(), slots, d_slot_c.get(), d_sums.get()));
      uint32_t nt32 = 0;
      NP_HIP(hipMemcpyAsync(&nt32, d_slot_c.get() + slots, 4, hipMemcpyDeviceToHost, st));
      NP_HIP(hipStreamSynchronize(st));
      n_terms = nt32;
      NP_TRY(W.take(rep_doc, n_terms, "the terms' documents"));
      NP_TRY(W.take(rep_rel, n_terms, "the terms' offsets"));
      NP_TRY(W.take(rep_len, n_terms, "the terms' lengths"));
      NP_TRY(W.take(d_rank, n_terms, "the terms' ranks"));
      hipLaunchKernelGGL(tb_compact, dim3(grid_of(slots, 256)), dim3(256), 0, st, (const uint32_t*)d_tab.get(),
                         (const uint32_t*)d_slot_c.get(), slots, (const uint32_t*)i_doc.get(), (const uint32_t*)i_rel.get(),
                         (const uint32_t*)i_len.get(), rep_doc.get(), rep_rel.get(), rep_len.get());
      NP_HIP(hipGetLastError());
      std::vector<uint32_t> h_doc((size_t)n_terms), h_rel((size_t)n_terms), h_len((size_t)n_terms), rank;
      NP_HIP(hipMemcpyAsync(h_doc.data(), rep_doc.get(), (size_t)n_terms * 4, hipMemcpyDeviceToHost, st));
      NP_HIP(hipMemcpyAsync(h_rel.data(), rep_rel.get(), (size_t)n_terms * 4, hipMemcpyDeviceToHost, st));
      NP_HIP(hipMemcpyAsync(h_len.data(), rep_len.get(), (size_t)n_terms * 4, hipMemcpyDeviceToHost, st));
      NP_HIP(hipStreamSynchronize(st));
      // the folded strings, out of the caller's own copy of the text, in the compacted order; then fts5vocab's order
      std::vector<uint8_t> raw;
      std::vector<int64_t> raw_off((size_t)n_terms + 1, 0);
      if (utf8) {   // through the caller's table, as the device compared them: marks go, a fold may change the length
        for (int64_t c = 0; c < n_terms; ++c) {
          textbuild_fold_utf8(bytes + offsets[h_doc[(size_t)c]] + h_rel[(size_t)c], h_len[(size_t)c], plan.unicode_table, &raw);
          raw_off[(size_t)c + 1] = (int64_t)raw.size();
        }
      } else {
        for (int64_t c = 0; c < n_terms; ++c) raw_off[(size_t)c + 1] = raw_off[(size_t)c] + h_len[(size_t)c];
        raw.resize((size_t)raw_off[(size_t)n_terms]);
        for (int64_t c = 0; c < n_terms; ++c) {
          const uint8_t* p = bytes + offsets[h_doc[(size_t)c]] + h_rel[(size_t)c];
          uint8_t* q = raw.data() + raw_off[(size_t)c];
          for (uint32_t i = 0; i < h_len[(size_t)c]; ++i) q[i] = textbuild_fold(p[i]);
        }
      }
      textbuild_sort_terms(raw.data(), raw_off.data(), n_terms, &rank, &B->term_bytes, &B->term_byte_offsets);
      NP_HIP(hipMemcpyAsync(d_rank.get(), rank.data(), (size_t)n_terms * 4, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(tb_assign_unicode, dim3(inst_grid), dim3(256), 0, st, key_a.get(), val_a.get(), n_inst,
                         (const uint32_t*)d_slot_c.get(), (const uint32_t*)d_rank.get());
      NP_HIP(hipGetLastError());
      NP_HIP(hipStreamSynchronize(st));   // rank (host memory) and the table's arrays go out of scope here
    } else {
      DevPtr<uint32_t> d_cnt, d_prefix;
      NP_TRY(W.take(d_cnt, bm_words, "the bitmap's counts"));
      NP_TRY(W.take(d_prefix, bm_words + 1, "the bitmap's prefix"));
      NP_TRY(need_sums(bm_words + 1));
      hipLaunchKernelGGL(tb_popc, dim3(grid_of(bm_words, 256)), dim3(256), 0, st, (const uint32_t*)d_bitmap.get(), bm_words,
                         d_cnt.get());
      NP_TRY(tb_scan<uint32_t>(st, d_cnt.get(), bm_words, d_prefix.get(), d_sums.get()));
      hipLaunchKernelGGL(tb_assign_trigram, dim3(inst_grid), dim3(256), 0, st, key_a.get(), val_a.get(), n_inst,
                         (const uint32_t*)d_bitmap.get(), (const uint32_t*)d_prefix.get());
      NP_HIP(hipGetLastError());
      std::vector<uint32_t> h_bm((size_t)bm_words);
      NP_HIP(hipMemcpyAsync(h_bm.data(), d_bitmap.get(), (size_t)bm_words * 4, hipMemcpyDeviceToHost, st));
      NP_HIP(hipStreamSynchronize(st));
      for (int64_t w = 0; w < bm_words; ++w)
        for (uint32_t m = h_bm[(size_t)w]; m; m &= m - 1) {
          const uint32_t k = (uint32_t)w * 32u + (uint32_t)__builtin_ctz(m);
          B->term_bytes.push_back((uint8_t)(k >> 14));
          B->term_bytes.push_back((uint8_t)((k >> 7) & 127u));
          B->term_bytes.push_back((uint8_t)(k & 127u));
          B->term_byte_offsets.push_back((int64_t)B->term_bytes.size());
        }
      n_terms = (int64_t)B->term_byte_offsets.size() - 1;
    }
    ms_terms = ms_since(t0);

    // ---- order
    t0 = Clock::now();
    passes = textbuild_sort_passes(n_terms);
    const int64_t nblk = (n_inst + NP_TB_SORT_CHUNK - 1) / NP_TB_SORT_CHUNK;
    DevPtr<uint32_t> d_hist;
    if (passes > 0) {
      NP_TRY(W.take(d_hist, 256 * nblk + 1, "the sort's histograms"));
      NP_TRY(need_sums(256 * nblk + 1));
    }
    uint32_t *ka = key_a.get(), *va = val_a.get(), *kb = key_b.get(), *vb = val_b.get();
    for (int p = 0; p < passes; ++p) {
      hipLaunchKernelGGL(tb_radix_hist, dim3((unsigned)nblk), dim3(64), 0, st, (const uint32_t*)ka, n_inst, p * 8, d_hist.get(), nblk);
      NP_TRY(tb_scan<uint32_t>(st, d_hist.get(), 256 * nblk, d_hist.get(), d_sums.get()));
      hipLaunchKernelGGL(tb_radix_scatter, dim3((unsigned)nblk), dim3(64), 0, st, (const uint32_t*)ka, (const uint32_t*)va, kb, vb,
                         n_inst, p * 8, (const uint32_t*)d_hist.get(), nblk);
      NP_HIP(hipGetLastError());
      std::swap(ka, kb);
      std::swap(va, vb);
    }
    NP_TRY(W.take(B->d_toff, n_terms + 1, "term_offsets"));
    NP_TRY(W.take(B->d_inst_doc, n_inst, "inst_doc"));
    NP_TRY(W.take(B->d_inst_pos, n_inst, "inst_pos"));
    hipLaunchKernelGGL(tb_gather, dim3(inst_grid), dim3(256), 0, st, (const uint32_t*)ka, (const uint32_t*)va, n_inst, n_terms,
                       (const uint32_t*)i_doc.get(), (const uint32_t*)i_rel.get(), (const int64_t*)d_first.get(), unicode ? 1 : 0,
                       B->d_inst_doc.get(), B->d_inst_pos.get(), B->d_toff.get());
    NP_HIP(hipGetLastError());
    NP_HIP(hipStreamSynchronize(st));
    ms_sort = ms_since(t0);
  }
  B->n_terms = n_terms;
  if (rep) {
    memset(rep, 0, sizeof(*rep));
    rep->n_docs = n_docs;
    rep->n_fallback = (int64_t)B->fallback.size();
    rep->n_instances = n_inst;
    rep->n_terms = n_terms;
    rep->term_bytes = (int64_t)B->term_bytes.size();
    rep->table_retries = retries;
    rep->sort_passes = passes;
    rep->hash_bits = bits;
    rep->tile_bytes = plan.tile_bytes;
    rep->ms_upload = ms_upload;
    rep->ms_classify = ms_classify;
    rep->ms_emit = ms_emit;
    rep->ms_terms = ms_terms;
    rep->ms_sort = ms_sort;
    rep->ms_total = ms_since(t_all);
    rep->workspace_bytes = W.held;
  }
  return NP_OK;
}

}  // namespace
}  // namespace np

extern "C" {

int np_hip_text_build(int32_t device, const uint8_t* bytes, const int64_t* offsets, int64_t n_docs, const np_text_build_opts* opts,
                      np_text_build** out_build, np_text_build_report* report) {
  clear_error();
  if (!out_build) {
    set_error("np_hip_text_build: out_build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out_build = nullptr;
  TextBuildPlan plan;
  char why[256];
  const int rc = textbuild_check_args(offsets, n_docs, opts, bytes != nullptr, &plan, why, sizeof(why));
  if (rc != NP_OK) {
    set_error(rc == NP_ERR_SHAPE ? "%s" : "np_hip_text_build: %s", why);
    return rc;
  }
  np_text_build* b = new (std::nothrow) np_text_build();
  if (!b) {
    set_error("np_hip_text_build: out of host memory");
    return NP_ERR_OUT_OF_MEMORY;
  }
  int rc2;
  try {
    rc2 = text_build_impl(device, bytes, offsets, n_docs, plan, b, report);
  } catch (const std::bad_alloc&) {
    set_error("np_hip_text_build: out of host memory");
    rc2 = NP_ERR_OUT_OF_MEMORY;
  }
  if (rc2 != NP_OK) {
    np_hip_text_build_free(b);
    return rc2;
  }
  *out_build = b;
  return NP_OK;
}

int np_hip_text_build_fallback(const np_text_build* build, int64_t* out_doc_ids, int64_t* out_count) {
  clear_error();
  if (!build) {
    set_error("np_hip_text_build_fallback: build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (out_count) *out_count = (int64_t)build->fallback.size();
  if (out_doc_ids && !build->fallback.empty()) memcpy(out_doc_ids, build->fallback.data(), build->fallback.size() * 8);
  return NP_OK;
}

int np_hip_text_build_add(np_text_build* build, const uint8_t* term_bytes, const int64_t* term_byte_offsets, int64_t n_terms,
                          const int32_t* inst_term, const int64_t* inst_doc, const int32_t* inst_pos, int64_t n) {
  clear_error();
  if (!build) {
    set_error("np_hip_text_build_add: build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (build->added || build->finalised) {
    set_error(build->added ? "np_hip_text_build_add: instances were added before; they may be added once"
                           : "np_hip_text_build_add: the sizes were read; instances are added before that");
    return NP_ERR_INVALID_ARGUMENT;
  }
  char why[256];
  const int rc = textbuild_check_added(term_bytes, term_byte_offsets, n_terms, inst_term, inst_doc, inst_pos, n,
                                       build->fallback.data(), (int64_t)build->fallback.size(), why, sizeof(why));
  if (rc != NP_OK) {
    set_error("np_hip_text_build_add: %s", why);
    return rc;
  }
  try {
    if (n_terms > 0) {
      build->b_bytes.assign(term_bytes, term_bytes + term_byte_offsets[n_terms]);
      build->b_tbo.assign(term_byte_offsets, term_byte_offsets + n_terms + 1);
    }
    build->b_term.assign(inst_term, inst_term + n);
    build->b_doc.assign(inst_doc, inst_doc + n);
    build->b_pos.assign(inst_pos, inst_pos + n);
  } catch (const std::bad_alloc&) {
    set_error("np_hip_text_build_add: out of host memory");
    return NP_ERR_OUT_OF_MEMORY;
  }
  build->added = true;
  return NP_OK;
}

static int tb_download(const np_text_build* b, int64_t* toff, int64_t* inst_doc, int32_t* inst_pos) {
  DeviceGuard g(b->device);
  if (toff) NP_HIP(hipMemcpy(toff, b->d_toff.get(), (size_t)(b->n_terms + 1) * 8, hipMemcpyDeviceToHost));
  if (inst_doc && b->n_inst > 0) NP_HIP(hipMemcpy(inst_doc, b->d_inst_doc.get(), (size_t)b->n_inst * 8, hipMemcpyDeviceToHost));
  if (inst_pos && b->n_inst > 0) NP_HIP(hipMemcpy(inst_pos, b->d_inst_pos.get(), (size_t)b->n_inst * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

int np_hip_text_build_sizes(np_text_build* build, int64_t* n_terms, int64_t* term_bytes, int64_t* n_instances, int64_t* n_rows) {
  clear_error();
  if (!build) {
    set_error("np_hip_text_build_sizes: build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!build->finalised) {
    if (build->added && !build->b_term.empty()) {
      try {
        TextArrays a;
        a.term_bytes = build->term_bytes;
        a.term_byte_offsets = build->term_byte_offsets;
        a.term_offsets.resize((size_t)build->n_terms + 1);
        a.inst_doc.resize((size_t)build->n_inst);
        a.inst_pos.resize((size_t)build->n_inst);
        NP_TRY(tb_download(build, a.term_offsets.data(), a.inst_doc.data(), a.inst_pos.data()));
        textbuild_merge(a, build->b_bytes.data(), build->b_tbo.data(), (int64_t)build->b_tbo.size() - 1, build->b_term.data(),
                        build->b_doc.data(), build->b_pos.data(), (int64_t)build->b_term.size(), &build->out);
      } catch (const std::bad_alloc&) {
        set_error("np_hip_text_build_sizes: out of host memory");
        return NP_ERR_OUT_OF_MEMORY;
      }
      build->merged = true;
      DeviceGuard g(build->device);
      build->d_toff.reset();
      build->d_inst_doc.reset();
      build->d_inst_pos.reset();
    }
    build->finalised = true;
  }
  if (n_terms) *n_terms = build->merged ? build->out.n_terms() : build->n_terms;
  if (term_bytes) *term_bytes = (int64_t)(build->merged ? build->out.term_bytes.size() : build->term_bytes.size());
  // (a consumed build gave its instance arrays away: the install left their count in n_inst)
  if (n_instances) *n_instances = build->merged && !build->consumed ? (int64_t)build->out.inst_doc.size() : build->n_inst;
  if (n_rows) *n_rows = build->n_docs;
  return NP_OK;
}

int np_hip_text_build_fetch(const np_text_build* build, uint8_t* term_bytes, int64_t* term_byte_offsets, int64_t* term_offsets,
                            int64_t* inst_doc, int32_t* inst_pos) {
  clear_error();
  if (!build || !build->finalised) {
    set_error(build ? "np_hip_text_build_fetch: call np_hip_text_build_sizes first" : "np_hip_text_build_fetch: build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const std::vector<uint8_t>& tb = build->merged ? build->out.term_bytes : build->term_bytes;
  const std::vector<int64_t>& tbo = build->merged ? build->out.term_byte_offsets : build->term_byte_offsets;
  if (term_bytes && !tb.empty()) memcpy(term_bytes, tb.data(), tb.size());
  if (term_byte_offsets) memcpy(term_byte_offsets, tbo.data(), tbo.size() * 8);
  if (build->consumed && (term_offsets || inst_doc || inst_pos)) {
    set_error("np_hip_text_build_fetch: %s: the build is consumed, np_hip_index_set_text_build gave its instance arrays to a handle "
              "(np_hip_index_get_text reads them back)",
              term_offsets ? "term_offsets" : inst_doc ? "inst_doc" : "inst_pos");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!build->merged) return tb_download(build, term_offsets, inst_doc, inst_pos);
  const TextArrays& o = build->out;
  if (term_offsets) memcpy(term_offsets, o.term_offsets.data(), o.term_offsets.size() * 8);
  if (inst_doc && !o.inst_doc.empty()) memcpy(inst_doc, o.inst_doc.data(), o.inst_doc.size() * 8);
  if (inst_pos && !o.inst_pos.empty()) memcpy(inst_pos, o.inst_pos.data(), o.inst_pos.size() * 4);
  return NP_OK;
}

void np_hip_text_build_free(np_text_build* build) {
  if (!build) return;
  DeviceGuard g(build->device);
  delete build;
}

}  // extern "C"
