// np_text.hip -- the keyword half of a hybrid search on the device: the FTS5 index in HBM (np_hip_index_set_text), BM25
// keyword search with SQLite's bits (np_hip_text_search), the fusion of a semantic and a keyword list (np_hip_fuse) and the
// whole hybrid request (np_hip_search_hybrid).
//
//   text_hit_kernel<PX>  nHit of every phrase of several tokens: the documents of the WHOLE table that hold it.  One lane per
//                      posting of the phrase's first token; text_block_count adds the block's count with one integer atomic
//                      (order cannot show).  <false>: flat queries; <true>: tree queries, whose last token may be a prefix
//   text_prefix_kernel a tree query's single-token prefix phrases: per-document frequencies over the term range, and nHit
//   text_score_kernel  a workgroup takes one (query, slice of NP_TEXT_SLICE_DOCS consecutive documents).  One f64 accumulator
//                      and one match count per document of the slice in LDS; the phrases are walked in order with a barrier
//                      between them, each lane takes one posting of the phrase's first token inside the slice (a document
//                      occurs once per posting list: lanes never collide, and phrase order is the summation order), reads the
//                      stored frequency or intersects positions, and adds the bm25 term.  The slice's matching, eligible
//                      documents are then sorted by (score, id) and the best `keep` leave as the slice's list
//   text_expr_kernel   the same for a tree query (np_text_expr): phrase masks, the node list per document, the live phrases' terms
//   text_merge_kernel  per query: the lists of a chunk's slices and the result of the chunks before it, merged through a
//                      2048-entry window in LDS by the same total order
//   fuse_kernel        per query: the two lists in LDS, the fused scores in f32 in the reference's order, one sort
//   text_rank_merge_kernel  per query: the sorted lists of G document shards into the global top-k by binary searches
// What must stay SQLite's bit for bit is written once and shared: text_bm25_term (the score's expression), text_probe and
// text_phrase_walk (a phrase's occurrences), and the two slice kernels' common ends -- text_slice, text_slice_range, text_in_subset,
// text_slice_emit.  On the host one TextProg lays out a flat or a tree batch and one text_run runs either.
// Over document shards (np_hip_index_set_text_shard, np_hip_text_search_sharded, np_hip_search_hybrid_sharded; np_dist_plan.h
// has the records): a shard keeps its slice of the table and the table's global figures, the shards' phrase hit counts are summed
// on the host before the idf is computed, and the shards' lists cross the ranks as f64 keys and global ids.
// The f64 arithmetic of a score is SQLite's expression, operation for operation (this file is compiled with
// -ffp-contract=off: no product and sum may be fused); the idf needs libm's log and is computed on the host.
#include "np_internal.h"
#include "np_dist_plan.h"
#include "np_text_plan.h"

#include <chrono>
#include <string.h>

namespace np {

constexpr int TEXT_TPB = 256;
constexpr int TEXT_SLICE = (int)NP_TEXT_SLICE_DOCS;
constexpr int TEXT_WINDOW = 2 * NP_TEXT_MAX_TOPK;   // entries of the merge window and of a fusion

struct TextIxP {
  const int64_t* post_off;
  const int32_t* post_doc;
  const int32_t* post_tf;
  const int64_t* post_first;
  const int32_t* pos;
  const int32_t* doc_len;
};

// first index in [lo, hi) of an ascending i32 array with a[i] >= v
__device__ __forceinline__ int64_t text_lower_bound(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The bm25 term of a phrase that occurs freq times in a document of doc_len tokens: SQLite's expression, operation for
// operation.  The one place where it is written: its order is the contract (the callers add it as acc = acc + term).
__device__ __forceinline__ double text_bm25_term(double idf, double freq, double doc_len, double avgdl) {
  const double k1 = 1.2, b = 0.75;
  const double a = freq, D = doc_len;
  return idf * ((a * (k1 + 1.0)) / (a + k1 * (1 - b + b * D / avgdl)));
}

// does `term` occur in `doc` at position `pos`?  *in_doc: the document holds the term at all
__device__ __forceinline__ bool text_probe(const TextIxP& t, int term, int doc, int64_t pos, bool* in_doc) {
  const int64_t e = t.post_off[term + 1];
  const int64_t jk = text_lower_bound(t.post_doc, t.post_off[term], e, doc);
  *in_doc = jk < e && t.post_doc[jk] == doc;
  if (!*in_doc) return false;
  const int64_t pe = t.post_first[jk] + t.post_tf[jk];
  const int64_t at = text_lower_bound(t.pos, t.post_first[jk], pe, pos);
  return at < pe && (int64_t)t.pos[at] == pos;
}

// occurrences of a phrase of several tokens in the document of posting j0 (a posting of terms[0]): positions p of terms[0] with
// terms[k] at p + k for every k.  PX: the last token stands for the terms [terms[nt - 1], hi) -- a position holds one term, so
// at most one term of the range continues an occurrence.
template <bool PX>
__device__ __forceinline__ int text_phrase_walk(const TextIxP& t, const int32_t* __restrict__ terms, int nt, int hi, int64_t j0, int doc) {
  const int tf0 = t.post_tf[j0];
  const int64_t f0 = t.post_first[j0];
  const int exact = PX ? nt - 1 : nt;   // the tokens [1, exact) are single terms
  int freq = 0;
  for (int x = 0; x < tf0; ++x) {
    const int64_t p = t.pos[f0 + x];
    bool ok = true, in_doc;
    for (int k = 1; k < exact && ok; ++k) {
      ok = text_probe(t, terms[k], doc, p + k, &in_doc);
      if (!in_doc) return 0;   // the document lacks a token of the phrase
    }
    if (PX && ok) {
      ok = false;
      for (int term = terms[nt - 1]; term < hi && !ok; ++term) ok = text_probe(t, term, doc, p + nt - 1, &in_doc);
    }
    freq += ok ? 1 : 0;
  }
  return freq;
}

// occurrences of the phrase terms[0 .. nt) in the document of posting j0: the stored frequency of a single token, else the walk
__device__ __forceinline__ int text_phrase_freq(const TextIxP& t, const int32_t* __restrict__ terms, int nt, int64_t j0, int doc) {
  return nt == 1 ? t.post_tf[j0] : text_phrase_walk<false>(t, terms, nt, 0, j0, doc);
}
// ... of a tree query's phrase: hi = 0 is the exact phrase (which takes the exact walk), else the end of the last token's range
__device__ __forceinline__ int text_phrase_freq_px(const TextIxP& t, const int32_t* __restrict__ terms, int nt, int hi, int64_t j0, int doc) {
  return hi == 0 || nt == 1 ? text_phrase_freq(t, terms, nt, j0, doc) : text_phrase_walk<true>(t, terms, nt, hi, j0, doc);
}

// The block's sum of c, added to *counter: a reduction per wave, the four waves' parts through LDS, one integer atomic (order
// cannot show).  Every thread of the block calls it, once.
__device__ __forceinline__ void text_block_count(uint32_t c, unsigned long long* counter) {
  __shared__ uint32_t part[TEXT_TPB / 64];
  const int tid = threadIdx.x;
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
  if ((tid & 63) == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    const uint32_t all = part[0] + part[1] + part[2] + part[3];
    if (all) atomicAdd(counter, (unsigned long long)all);
  }
}

struct TextHitP {
  TextIxP t;
  const int32_t* phr_tok;
  const int32_t* terms;
  const int32_t* phr_hi;           // [phrases] end of the last token's term range, 0 = exact; read by text_hit_kernel<true> only
  const int32_t* item_phr;         // [items] phrases of several known tokens
  unsigned long long* nhit;        // [items]
};

// nHit of a phrase of several tokens: the documents of the WHOLE table that hold it.  PX: the phrases of tree queries, whose last
// token may be a prefix; text_hit_kernel<false> is the flat queries' and knows nothing of prefixes.
template <bool PX>
__global__ void __launch_bounds__(TEXT_TPB) text_hit_kernel(TextHitP p) {
  const int item = blockIdx.y, tid = threadIdx.x;
  const int phr = p.item_phr[item];
  const int tb = p.phr_tok[phr], nt = p.phr_tok[phr + 1] - tb;
  const int32_t* terms = p.terms + tb;
  const int hi_t = PX ? p.phr_hi[phr] : 0;
  const int64_t lo = p.t.post_off[terms[0]], hi = p.t.post_off[terms[0] + 1];
  uint32_t c = 0;
  for (int64_t j = lo + (int64_t)blockIdx.x * TEXT_TPB + tid; j < hi; j += (int64_t)gridDim.x * TEXT_TPB) {
    const int doc = p.t.post_doc[j];
    c += (PX ? text_phrase_freq_px(p.t, terms, nt, hi_t, j, doc) : text_phrase_freq(p.t, terms, nt, j, doc)) > 0 ? 1u : 0u;
  }
  text_block_count(c, &p.nhit[item]);
}

struct TextPrefixP {
  TextIxP t;
  const int32_t* phr_tok;
  const int32_t* terms;
  const int32_t* phr_hi;
  const int32_t* px_phr;           // [prefix phrases of the chunk] single-token phrases that end in a prefix
  const int32_t* px_at;            // [the same] the phrase's frequency array: (query of the chunk) * slots + slot
  uint32_t* pfreq;                 // [chunk queries * slots][stride] zeroed
  int64_t stride;
  unsigned long long* pxhit;       // [phrases] zeroed
};

// The pre-pass of a single-token prefix phrase: the postings of the terms [lo, hi) are ONE run of the posting arrays; a lane
// per posting adds the term frequency to the document's entry (integer adds: order cannot show).  The lane that finds the
// entry at zero counts the document: nHit = documents that hold any term of the range.
__global__ void __launch_bounds__(TEXT_TPB) text_prefix_kernel(TextPrefixP p) {
  const int tid = threadIdx.x;
  const int phr = p.px_phr[blockIdx.y];
  const int term = p.terms[p.phr_tok[phr]];
  uint32_t* arr = p.pfreq + (int64_t)p.px_at[blockIdx.y] * p.stride;
  const int64_t lo = p.t.post_off[term], hi = p.t.post_off[p.phr_hi[phr]];
  uint32_t c = 0;
  for (int64_t j = lo + (int64_t)blockIdx.x * TEXT_TPB + tid; j < hi; j += (int64_t)gridDim.x * TEXT_TPB)
    c += atomicAdd(&arr[p.t.post_doc[j]], (uint32_t)p.t.post_tf[j]) == 0u ? 1u : 0u;   // (a posting's frequency is >= 1)
  text_block_count(c, &p.pxhit[phr]);
}

struct TextPrefixCountP {
  TextIxP t;
  const int32_t* phr_tok;
  const int32_t* terms;
  const int32_t* phr_hi;
  const int32_t* px_phr;           // [prefix phrases of the group]
  uint32_t* bits;                  // [group][words] zeroed: one bit per document of the shard
  int64_t words;
  unsigned long long* nhit;        // [group] zeroed
};

// nHit of a single-token prefix phrase and nothing else: the counting pre-pass of a sharded tree batch, which runs for the
// whole batch ahead of the chunk loop (the counts cross the ranks before any idf is computed; text_prefix_kernel still fills
// the frequency arrays per chunk).  A lane per posting of the run [post_off[lo], post_off[hi]) sets its document's bit; the
// lane that finds it clear counts the document.  The words are global: a run is sorted by document inside a term only, so a
// workgroup's postings spread over the whole shard and no slice of the bitmap fits LDS; the L2 resolves the atomics, and a
// bit per document keeps a group's bitmaps inside it.  Integer atomics only: order cannot show.  No workgroup waits for another.
__global__ void __launch_bounds__(TEXT_TPB) text_prefix_count_kernel(TextPrefixCountP p) {
  const int tid = threadIdx.x;
  const int phr = p.px_phr[blockIdx.y];
  const int term = p.terms[p.phr_tok[phr]];
  uint32_t* bits = p.bits + (int64_t)blockIdx.y * p.words;
  const int64_t lo = p.t.post_off[term], hi = p.t.post_off[p.phr_hi[phr]];
  uint32_t c = 0;
  for (int64_t j = lo + (int64_t)blockIdx.x * TEXT_TPB + tid; j < hi; j += (int64_t)gridDim.x * TEXT_TPB) {
    const int doc = p.t.post_doc[j];
    const uint32_t bit = 1u << (doc & 31);
    c += (atomicOr(&bits[doc >> 5], bit) & bit) == 0u ? 1u : 0u;
  }
  text_block_count(c, &p.nhit[blockIdx.y]);
}

// ---- the (query, slice) kernels: what the flat and the tree kernel share ------------------------------------------------------

struct TextScoreP {
  TextIxP t;
  const int32_t* q_phr;      // [B + 1] a query's phrases
  const int32_t* phr_tok;    // [phrases + 1] a phrase's tokens
  const int32_t* terms;
  const double* idf;         // [phrases]
  const int32_t* mode;       // [B]
  int64_t n_docs;
  double avgdl;
  int keep;                  // entries a slice hands on
  const uint32_t* docbits;   // [rows][NW]
  int64_t NW;
  int64_t S;                 // slices per query in the lists (the plan's)
  unsigned long long* list_keys;   // [chunk queries][S][keep] bits of the f64 score (positive: they order as integers)
  int32_t* list_ids;
  int32_t* list_cnt;         // [chunk queries][S]
  unsigned long long* ctr;   // postings visited, or NULL
  // what changes from launch to launch of a call
  int q0;                    // first query of the chunk
  int64_t s0;                // first slice of the chunk
  const int32_t* qrow;       // [chunk queries] row of docbits, -1 = no subset; NULL = no subsets at all
};

// the workgroup's (query, slice)
struct TextSlice {
  int64_t d0;     // first document of the slice
  int n;          // its documents
  int ph0, nph;   // the query's phrases
  int row;        // the query's row of docbits, -1 = no subset
  int64_t o;      // the (query, slice) pair in the lists
};

__device__ __forceinline__ TextSlice text_slice(const TextScoreP& p) {
  const int ql = blockIdx.y, q = p.q0 + ql;
  const int64_t sl = blockIdx.x;
  TextSlice s;
  s.d0 = (p.s0 + sl) * TEXT_SLICE;
  s.n = p.n_docs - s.d0 < TEXT_SLICE ? (int)(p.n_docs - s.d0) : TEXT_SLICE;
  s.ph0 = p.q_phr[q];
  s.nph = p.q_phr[q + 1] - s.ph0;
  s.row = p.qrow ? p.qrow[ql] : -1;
  s.o = (int64_t)ql * p.S + sl;
  return s;
}

// every token of the phrase is in the vocabulary
__device__ __forceinline__ bool text_phrase_known(const TextScoreP& p, int phr) {
  bool known = true;
  for (int k = p.phr_tok[phr]; k < p.phr_tok[phr + 1]; ++k) known = known && p.terms[k] >= 0;
  return known;
}

// the slice's part [*lo, *hi) of the phrase's first posting list; empty where a token of the phrase is unknown
__device__ __forceinline__ void text_slice_range(const TextScoreP& p, const TextSlice& s, int phr, int64_t* lo, int64_t* hi) {
  *lo = *hi = 0;
  if (!text_phrase_known(p, phr)) return;
  const int term = p.terms[p.phr_tok[phr]];
  const int64_t e = p.t.post_off[term + 1];
  *lo = text_lower_bound(p.t.post_doc, p.t.post_off[term], e, s.d0);
  *hi = text_lower_bound(p.t.post_doc, *lo, e, s.d0 + s.n);
}

// document i of the slice is in the subset of the query (one that has a subset: s.row >= 0)
__device__ __forceinline__ bool text_in_subset(const TextScoreP& p, const TextSlice& s, int i) {
  const int64_t d = s.d0 + i;
  return ((p.docbits[(int64_t)s.row * p.NW + (d >> 5)] >> (d & 31)) & 1u) != 0;
}

// The slice's list leaves: s_idx[0 .. nm) holds the matching documents' indexes in any order, s_acc their scores.  Bitonic sort
// of the indexes, padded to a power of two with 0xFFFF: score descending (a match's score is positive: its bits order as
// integers), then id; the best `keep` are written.  nm = 0: the empty list.  Every thread of the block calls it (block-uniform
// nm), behind a barrier after the last write to s_acc and s_idx.
__device__ __forceinline__ void text_slice_emit(const TextScoreP& p, const TextSlice& s, const double* s_acc, uint16_t* s_idx, int nm) {
  const int tid = threadIdx.x;
  if (nm == 0) {
    if (tid == 0) p.list_cnt[s.o] = 0;
    return;
  }
  int P2 = 1;
  while (P2 < nm) P2 <<= 1;
  for (int i = nm + tid; i < P2; i += TEXT_TPB) s_idx[i] = 0xFFFF;
  auto before = [&](uint16_t x, uint16_t y) {
    if (x == 0xFFFF) return false;
    if (y == 0xFFFF) return true;
    const unsigned long long kx = (unsigned long long)__double_as_longlong(s_acc[x]), ky = (unsigned long long)__double_as_longlong(s_acc[y]);
    return kx > ky || (kx == ky && x < y);
  };
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < P2; i += TEXT_TPB) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint16_t x = s_idx[i], y = s_idx[ixj];
          if ((i & k) == 0 ? before(y, x) : before(x, y)) {
            s_idx[i] = y;
            s_idx[ixj] = x;
          }
        }
      }
    }
  __syncthreads();
  const int kept = min(nm, p.keep);
  for (int r = tid; r < kept; r += TEXT_TPB) {
    const int l = s_idx[r];
    p.list_keys[s.o * p.keep + r] = (unsigned long long)__double_as_longlong(s_acc[l]);
    p.list_ids[s.o * p.keep + r] = (int32_t)(s.d0 + l);
  }
  if (tid == 0) p.list_cnt[s.o] = kept;
}

// ---- flat queries -----------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(TEXT_TPB) text_score_kernel(TextScoreP p) {
  __shared__ double s_acc[TEXT_SLICE];
  __shared__ uint8_t s_cnt[TEXT_SLICE];
  __shared__ uint16_t s_idx[TEXT_SLICE];
  __shared__ int64_t s_lo[NP_TEXT_MAX_PHRASES], s_hi[NP_TEXT_MAX_PHRASES];
  __shared__ int s_any, s_all, s_n;
  const int tid = threadIdx.x;
  const TextSlice s = text_slice(p);
  const int64_t d0 = s.d0;
  const int n = s.n, ph0 = s.ph0, nph = s.nph;
  if (tid == 0) {
    s_any = 0;
    s_all = 1;
    s_n = 0;
  }
  __syncthreads();
  if (tid < nph) {
    int64_t lo, hi;
    text_slice_range(p, s, ph0 + tid, &lo, &hi);
    s_lo[tid] = lo;
    s_hi[tid] = hi;
    if (hi > lo) atomicOr(&s_any, 1); else atomicAnd(&s_all, 0);
  }
  __syncthreads();
  const bool is_and = p.mode[p.q0 + blockIdx.y] == NP_TEXT_AND;
  if (!s_any || (is_and && !s_all)) return text_slice_emit(p, s, s_acc, s_idx, 0);   // (block-uniform) nothing of the slice can match
  for (int i = tid; i < n; i += TEXT_TPB) {
    s_acc[i] = 0.0;
    s_cnt[i] = 0;
  }
  __syncthreads();
  unsigned long long visited = 0;
  for (int ph = 0; ph < nph; ++ph) {
    const int64_t lo = s_lo[ph], hi = s_hi[ph];
    const int tb = p.phr_tok[ph0 + ph], nt = p.phr_tok[ph0 + ph + 1] - tb;
    const double idf = p.idf[ph0 + ph];
    for (int64_t j = lo + tid; j < hi; j += TEXT_TPB) {
      const int doc = p.t.post_doc[j];
      const int freq = text_phrase_freq(p.t, p.terms + tb, nt, j, doc);
      if (freq > 0) {
        const int l = (int)(doc - d0);
        s_acc[l] = s_acc[l] + text_bm25_term(idf, (double)freq, (double)p.t.doc_len[doc], p.avgdl);
        s_cnt[l] = (uint8_t)(s_cnt[l] + 1);
      }
    }
    visited += (unsigned long long)(hi - lo);
    __syncthreads();
  }
  if (p.ctr && tid == 0 && visited) atomicAdd(p.ctr, visited);
  // the slice's matching documents in scope: slots from a counter, the order from the sort in text_slice_emit
  for (int i = tid; i < n; i += TEXT_TPB) {
    bool m = is_and ? s_cnt[i] == nph : s_cnt[i] > 0;
    if (m && s.row >= 0) m = text_in_subset(p, s, i);
    if (m) s_idx[atomicAdd(&s_n, 1)] = (uint16_t)i;
  }
  __syncthreads();
  text_slice_emit(p, s, s_acc, s_idx, s_n);
}

// ---- tree queries (np_text_expr) ------------------------------------------------------------------------------------------

struct TextExprP {
  TextScoreP s;                    // text_score_kernel's arguments (mode is not read)
  const int32_t* phr_hi;           // [phrases]
  const int32_t* phr_slot;         // [phrases] a single-token prefix phrase's frequency array of its query, else -1
  const int32_t* q_node;           // [B + 1] a query's nodes
  const int32_t* nodes;            // op | a << 8 | b << 16, postfix
  const uint32_t* pfreq;           // [chunk queries * slots][stride]
  int64_t stride;
  int slots;
};

// text_score_kernel's decomposition and lists for a tree query.  Per document of the slice a 64-bit mask of the phrases that
// occur (pass 1, a phrase at a time as the scoring pass walks them); a lane per document then evaluates the nodes bottom-up,
// propagates liveness from the root down (a child is live if its parent is and the child is true; never the right child of a
// NOT) and leaves the mask of the LIVE phrases; pass 2 walks the phrases again, in order, and adds the bm25 term where the
// phrase is live -- the frequency of a phrase of several tokens is computed a second time, for live documents only.
// LDS: 32 KB accumulators, 32 KB masks, 8 KB sort index: two workgroups per CU.
__global__ void __launch_bounds__(TEXT_TPB) text_expr_kernel(TextExprP e) {
  __shared__ double s_acc[TEXT_SLICE];
  __shared__ unsigned long long s_mask[TEXT_SLICE];
  __shared__ uint16_t s_idx[TEXT_SLICE];
  __shared__ int64_t s_lo[NP_TEXT_MAX_PHRASES], s_hi[NP_TEXT_MAX_PHRASES];
  __shared__ int32_t s_node[NP_TEXT_MAX_NODES + 1];
  __shared__ int s_any, s_n;
  const TextScoreP& p = e.s;
  const int tid = threadIdx.x, ql = blockIdx.y, q = p.q0 + ql;
  const TextSlice s = text_slice(p);
  const int64_t d0 = s.d0;
  const int n = s.n, ph0 = s.ph0, nph = s.nph;
  const int nd0 = e.q_node[q], nn = e.q_node[q + 1] - nd0;
  if (tid == 0) {
    s_any = 0;
    s_n = 0;
  }
  __syncthreads();
  if (tid < nph) {
    int64_t lo = 0, hi = 0;
    if (e.phr_slot[ph0 + tid] >= 0) {   // (its documents are in the frequency array, not in one posting list)
      if (text_phrase_known(p, ph0 + tid)) atomicOr(&s_any, 1);
    } else {
      text_slice_range(p, s, ph0 + tid, &lo, &hi);
      if (hi > lo) atomicOr(&s_any, 1);
    }
    s_lo[tid] = lo;
    s_hi[tid] = hi;
  }
  for (int i = tid; i < nn; i += TEXT_TPB) s_node[i] = e.nodes[nd0 + i];
  __syncthreads();
  if (!s_any) return text_slice_emit(p, s, s_acc, s_idx, 0);   // (block-uniform) a match has a phrase that occurs
  for (int i = tid; i < n; i += TEXT_TPB) {
    s_acc[i] = 0.0;
    s_mask[i] = 0ull;
  }
  __syncthreads();
  unsigned long long visited = 0;
  // pass 1: the phrases that occur.  A document occurs once per posting list: lanes never collide inside a phrase
  for (int ph = 0; ph < nph; ++ph) {
    const unsigned long long bit = 1ull << ph;
    const int slot = e.phr_slot[ph0 + ph];
    if (slot >= 0) {
      const uint32_t* arr = e.pfreq + ((int64_t)ql * e.slots + slot) * e.stride + d0;
      for (int i = tid; i < n; i += TEXT_TPB)
        if (arr[i] > 0u) s_mask[i] |= bit;
    } else {
      const int64_t lo = s_lo[ph], hi = s_hi[ph];
      const int tb = p.phr_tok[ph0 + ph], nt = p.phr_tok[ph0 + ph + 1] - tb;
      const int hi_t = e.phr_hi[ph0 + ph];
      for (int64_t j = lo + tid; j < hi; j += TEXT_TPB) {
        const int doc = p.t.post_doc[j];
        if (text_phrase_freq_px(p.t, p.terms + tb, nt, hi_t, j, doc) > 0) s_mask[doc - d0] |= bit;
      }
      visited += (unsigned long long)(hi - lo);
    }
    __syncthreads();
  }
  if (p.ctr && tid == 0 && visited) atomicAdd(p.ctr, visited);
  // the tree, a lane per document: node truths bottom-up, liveness top-down, the live phrases back into the mask; the
  // matching documents in scope take their slots from a counter, the order comes from the sort in text_slice_emit
  for (int i = tid; i < n; i += TEXT_TPB) {
    const unsigned long long occ = s_mask[i];
    unsigned long long t0 = 0, t1 = 0;   // truth of the nodes 0..63 and 64..126
    auto truth = [&](int x) { return (int)(((x < 64 ? t0 : t1) >> (x & 63)) & 1ull); };
    for (int x = 0; x < nn; ++x) {
      const int32_t nd = s_node[x];
      const int op = nd & 0xFF, a = (nd >> 8) & 0xFF, b = (nd >> 16) & 0xFF;
      int v;
      if (op == NP_TEXT_NODE_PHRASE) v = (int)((occ >> a) & 1ull);
      else if (op == NP_TEXT_NODE_AND) v = truth(a) & truth(b);
      else if (op == NP_TEXT_NODE_OR) v = truth(a) | truth(b);
      else v = truth(a) & (truth(b) ^ 1);
      if (v) {
        if (x < 64) t0 |= 1ull << x; else t1 |= 1ull << (x & 63);
      }
    }
    bool m = occ != 0ull && truth(nn - 1) != 0;
    if (m && s.row >= 0) m = text_in_subset(p, s, i);
    unsigned long long live = 0;
    if (m) {
      unsigned long long l0 = 0, l1 = 0;   // liveness of the nodes
      if (nn - 1 < 64) l0 = 1ull << (nn - 1); else l1 = 1ull << ((nn - 1) & 63);
      for (int x = nn - 1; x >= 0; --x) {
        if (!(((x < 64 ? l0 : l1) >> (x & 63)) & 1ull)) continue;
        const int32_t nd = s_node[x];
        const int op = nd & 0xFF, a = (nd >> 8) & 0xFF, b = (nd >> 16) & 0xFF;
        if (op == NP_TEXT_NODE_PHRASE) {
          live |= 1ull << a;
          continue;
        }
        if (truth(a)) {
          if (a < 64) l0 |= 1ull << a; else l1 |= 1ull << (a & 63);
        }
        if (op != NP_TEXT_NODE_NOT && truth(b)) {
          if (b < 64) l0 |= 1ull << b; else l1 |= 1ull << (b & 63);
        }
      }
      s_idx[atomicAdd(&s_n, 1)] = (uint16_t)i;
    }
    s_mask[i] = live;
  }
  __syncthreads();
  const int nm = s_n;
  if (nm == 0) return text_slice_emit(p, s, s_acc, s_idx, 0);
  // pass 2: the bm25 terms of the live phrases, in phrase order (a live phrase has a positive term: a match's score is positive)
  for (int ph = 0; ph < nph; ++ph) {
    const double idf = p.idf[ph0 + ph];
    const int slot = e.phr_slot[ph0 + ph];
    if (slot >= 0) {
      const uint32_t* arr = e.pfreq + ((int64_t)ql * e.slots + slot) * e.stride + d0;
      for (int i = tid; i < n; i += TEXT_TPB)
        if ((s_mask[i] >> ph) & 1ull) s_acc[i] = s_acc[i] + text_bm25_term(idf, (double)arr[i], (double)p.t.doc_len[d0 + i], p.avgdl);
    } else {
      const int64_t lo = s_lo[ph], hi = s_hi[ph];
      const int tb = p.phr_tok[ph0 + ph], nt = p.phr_tok[ph0 + ph + 1] - tb;
      const int hi_t = e.phr_hi[ph0 + ph];
      for (int64_t j = lo + tid; j < hi; j += TEXT_TPB) {
        const int doc = p.t.post_doc[j];
        const int l = (int)(doc - d0);
        if ((s_mask[l] >> ph) & 1ull) {
          const int freq = text_phrase_freq_px(p.t, p.terms + tb, nt, hi_t, j, doc);
          s_acc[l] = s_acc[l] + text_bm25_term(idf, (double)freq, (double)p.t.doc_len[doc], p.avgdl);
        }
      }
    }
    __syncthreads();
  }
  text_slice_emit(p, s, s_acc, s_idx, nm);
}

// (key descending, id ascending) over the first `fill` entries of a window; entries up to the next power of two are padded
// with key 0 (no match has it).  Returns min(fill, top_k).  Every thread of the block calls it.
__device__ int text_sort_cut(unsigned long long* s_k, int32_t* s_i, int fill, int top_k, int tid) {
  int P2 = 1;
  while (P2 < fill) P2 <<= 1;
  __syncthreads();
  for (int i = fill + tid; i < P2; i += TEXT_TPB) {
    s_k[i] = 0ull;
    s_i[i] = 0x7FFFFFFF;
  }
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < P2; i += TEXT_TPB) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long ka = s_k[i], kb = s_k[ixj];
          const int32_t ia = s_i[i], ib = s_i[ixj];
          const bool a_first = ka > kb || (ka == kb && ia < ib);
          const bool b_first = kb > ka || (ka == kb && ib < ia);
          if ((i & k) == 0 ? b_first : a_first) {
            s_k[i] = kb;
            s_i[i] = ib;
            s_k[ixj] = ka;
            s_i[ixj] = ia;
          }
        }
      }
    }
  __syncthreads();
  return min(fill, top_k);
}

struct TextMergeP {
  const unsigned long long* list_keys;
  const int32_t* list_ids;
  const int32_t* list_cnt;
  int64_t S, Sn;             // slices per query in the lists; slices of this chunk
  int keep;
  int n_prev;                // 0 on a query's first chunk of slices, else best[] holds the result so far
  unsigned long long* best_keys;   // [chunk queries][top_k]
  int32_t* best_ids;
  int32_t* best_cnt;
  int top_k;
  int64_t* out_ids;          // [chunk queries][top_k]
  float* out_scores;
  int32_t* out_counts;
  unsigned long long* out_keys;   // [chunk queries][top_k] the f64 bits behind out_scores, or NULL (a shard's list needs them)
  int64_t id_base;           // added to the ids that leave: a shard's documents carry shard-local ids up to here
};

__global__ void __launch_bounds__(TEXT_TPB) text_merge_kernel(TextMergeP p) {
  __shared__ unsigned long long s_k[TEXT_WINDOW];
  __shared__ int32_t s_i[TEXT_WINDOW];
  const int b = blockIdx.x, tid = threadIdx.x;
  int fill = 0;
  if (p.n_prev) {
    fill = p.best_cnt[b];
    for (int i = tid; i < fill; i += TEXT_TPB) {
      s_k[i] = p.best_keys[(int64_t)b * p.top_k + i];
      s_i[i] = p.best_ids[(int64_t)b * p.top_k + i];
    }
  }
  for (int64_t s = 0; s < p.Sn; ++s) {
    const int64_t o = (int64_t)b * p.S + s;
    const int c = p.list_cnt[o];   // block-uniform; at most keep <= 1024, and top_k + keep fits the window
    if (c == 0) continue;
    if (fill + c > TEXT_WINDOW) fill = text_sort_cut(s_k, s_i, fill, p.top_k, tid);
    for (int i = tid; i < c; i += TEXT_TPB) {
      s_k[fill + i] = p.list_keys[o * p.keep + i];
      s_i[fill + i] = p.list_ids[o * p.keep + i];
    }
    fill += c;
  }
  fill = text_sort_cut(s_k, s_i, fill, p.top_k, tid);
  for (int j = tid; j < p.top_k; j += TEXT_TPB) {
    const int64_t at = (int64_t)b * p.top_k + j;
    const bool in = j < fill;
    p.best_keys[at] = in ? s_k[j] : 0ull;
    p.best_ids[at] = in ? s_i[j] : 0;
    p.out_ids[at] = in ? (int64_t)s_i[j] + p.id_base : 0;
    p.out_scores[at] = in ? (float)__longlong_as_double((long long)s_k[j]) : 0.f;
    if (p.out_keys) p.out_keys[at] = in ? s_k[j] : 0ull;
  }
  if (tid == 0) {
    p.best_cnt[b] = fill;
    p.out_counts[b] = fill;
  }
}

// ---- the merge of the shards' lists (np_hip_text_search_sharded) ------------------------------------------------------------
// One record per rank, rec_bytes apart (np_dist_plan.h, dist_text_record): keys [B][top_k] u64 at 0, global ids [B][top_k] i64 at
// o_ids, counts [B] i32 at o_counts, the status word at o_status.
struct TextRankMergeP {
  const char* rec;
  int64_t rec_bytes, o_ids, o_counts, o_status;
  int G, top_k;
  int64_t* out_ids;          // [B][top_k]
  float* out_scores;
  int32_t* out_counts;
  unsigned long long* host_status;   // pinned host memory or NULL: where a failed rank's word is left (np_hip_comm_status)
};

// entries of a list of n, sorted by (key descending, id ascending), that precede (key, id) under that order
__device__ __forceinline__ int text_rank_before(const unsigned long long* __restrict__ k, const int64_t* __restrict__ ids, int n,
                                                unsigned long long key, int64_t id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned long long km = k[mid];
    if (km > key || (km == key && ids[mid] < id)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One block per query: G lists of at most top_k entries, each already sorted by the total order (f64 score descending, global id
// ascending; the shards' ids are disjoint), into the global top-k.  An entry's place is its own index plus, for every other
// rank's list, the number of entries that precede it there -- one binary search per list, straight from the gathered records:
// no LDS, no atomics, no limit on G x top_k, the same bits from run to run.  A non-zero status word of any rank abandons every
// query of the batch (count -1) as the semantic merge does.
__global__ void __launch_bounds__(TEXT_TPB) text_rank_merge_kernel(TextRankMergeP p) {
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long failed = 0;
  for (int g = 0; g < p.G && !failed; ++g) failed = *(const unsigned long long*)(p.rec + (int64_t)g * p.rec_bytes + p.o_status);
  if (failed) {   // block-uniform: every thread read the same words
    if (tid == 0) {
      p.out_counts[b] = NP_COUNT_ABANDONED;
      if (b == 0 && p.host_status) *p.host_status = failed;
    }
    return;
  }
  auto count_of = [&](int g) {
    const int c = ((const int32_t*)(p.rec + (int64_t)g * p.rec_bytes + p.o_counts))[b];
    return max(0, min(c, p.top_k));
  };
  int total = 0;
  for (int g = 0; g < p.G; ++g) total += count_of(g);
  const int64_t row = (int64_t)b * p.top_k;
  for (int i = tid; i < p.G * p.top_k; i += TEXT_TPB) {
    const int g = i / p.top_k, j = i - g * p.top_k;
    if (j >= count_of(g)) continue;
    const char* mine = p.rec + (int64_t)g * p.rec_bytes;
    const unsigned long long key = ((const unsigned long long*)mine)[row + j];
    const int64_t id = ((const int64_t*)(mine + p.o_ids))[row + j];
    int at = j;
    for (int g2 = 0; g2 < p.G && at < p.top_k; ++g2) {
      if (g2 == g) continue;
      const char* other = p.rec + (int64_t)g2 * p.rec_bytes;
      at += text_rank_before((const unsigned long long*)other + row, (const int64_t*)(other + p.o_ids) + row, count_of(g2), key, id);
    }
    if (at < p.top_k) {
      p.out_ids[row + at] = id;
      p.out_scores[row + at] = (float)__longlong_as_double((long long)key);
    }
  }
  const int fill = min(total, p.top_k);
  for (int j = fill + tid; j < p.top_k; j += TEXT_TPB) {
    p.out_ids[row + j] = 0;
    p.out_scores[row + j] = 0.f;
  }
  if (tid == 0) p.out_counts[b] = fill;
}

// ---- fusion ------------------------------------------------------------------------------------------------------------
struct FuseP {
  int mode;
  float alpha;
  int top_k;
  const int64_t* sem_ids;
  const float* sem_sc;
  const int32_t* sem_cnt;
  int sem_stride;
  const int64_t* kw_ids;
  const float* kw_sc;
  const int32_t* kw_cnt;
  int kw_stride;
  int64_t* out_ids;
  float* out_sc;
  int32_t* out_cnt;
};

// min and max of a list ignoring NaN (f32::min / max), to every thread; INFINITY / -INFINITY for a list of NaNs
__device__ void fuse_min_max(const float* __restrict__ v, int n, float* s_red, float* mn, float* mx) {
  const int tid = threadIdx.x;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < n; i += TEXT_TPB) {
    lo = fminf(lo, v[i]);
    hi = fmaxf(hi, v[i]);
  }
  for (int s = 32; s > 0; s >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, s));
    hi = fmaxf(hi, __shfl_xor(hi, s));
  }
  __syncthreads();
  if ((tid & 63) == 0) {
    s_red[tid >> 6] = lo;
    s_red[4 + (tid >> 6)] = hi;
  }
  __syncthreads();
  *mn = fminf(fminf(s_red[0], s_red[1]), fminf(s_red[2], s_red[3]));
  *mx = fmaxf(fmaxf(s_red[4], s_red[5]), fmaxf(s_red[6], s_red[7]));
}

// a fused score as an integer that orders like it: NaN lowest, then -inf .. +inf (both zeros alike); 0 is left for padding
__device__ __forceinline__ uint32_t fuse_order(float s) {
  if (s != s) return 1u;
  if (s == 0.0f) s = 0.0f;
  const uint32_t u = __float_as_uint(s);
  return ((u & 0x80000000u) ? ~u : (u | 0x80000000u)) + 1u;
}

__global__ void __launch_bounds__(TEXT_TPB) fuse_kernel(FuseP p) {
  __shared__ int64_t s_id[TEXT_WINDOW];
  __shared__ float s_sc[TEXT_WINDOW];
  __shared__ uint32_t s_key[TEXT_WINDOW];
  __shared__ float s_red[8];
  __shared__ int s_n;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int ns = max(0, min(p.sem_cnt[b], p.sem_stride)), nk = max(0, min(p.kw_cnt[b], p.kw_stride));
  const int64_t* sid = p.sem_ids + (int64_t)b * p.sem_stride;
  const int64_t* kid = p.kw_ids + (int64_t)b * p.kw_stride;
  const float* ssc = p.sem_sc ? p.sem_sc + (int64_t)b * p.sem_stride : nullptr;
  const float* ksc = p.kw_sc ? p.kw_sc + (int64_t)b * p.kw_stride : nullptr;
  const bool rrf = p.mode == NP_FUSE_RRF;
  const float alpha = p.alpha, beta = 1.0f - p.alpha;
  float smin = 0.f, smax = 0.f, kmin = 0.f, kmax = 0.f;
  if (!rrf) {
    fuse_min_max(ssc, ns, s_red, &smin, &smax);
    fuse_min_max(ksc, nk, s_red, &kmin, &kmax);
  }
  if (tid == 0) s_n = ns;
  for (int r = tid; r < ns; r += TEXT_TPB) {
    float x;
    if (rrf) {
      x = alpha / (60.0f + (float)r + 1.0f);
    } else {
      const float nrm = smax == smin ? 1.0f : (ssc[r] - smin) / (smax - smin);
      x = alpha * nrm;
    }
    s_id[r] = sid[r];
    s_sc[r] = 0.0f + x;
  }
  __syncthreads();
  for (int r = tid; r < nk; r += TEXT_TPB) {
    float y;
    if (rrf) {
      y = beta / (60.0f + (float)r + 1.0f);
    } else {
      const float nrm = kmax == kmin ? 1.0f : (ksc[r] - kmin) / (kmax - kmin);
      y = beta * nrm;
    }
    const int64_t id = kid[r];
    int m = -1;
    for (int i = 0; i < ns; ++i)
      if (s_id[i] == id) {
        m = i;
        break;
      }
    if (m >= 0) {   // (an id occurs once per list: no other lane has this entry)
      s_sc[m] = s_sc[m] + y;
    } else {        // slots from a counter, the order from the sort below
      const int at = atomicAdd(&s_n, 1);
      s_id[at] = id;
      s_sc[at] = 0.0f + y;
    }
  }
  __syncthreads();
  const int n = s_n;
  int P2 = 1;
  while (P2 < n) P2 <<= 1;
  for (int i = tid; i < P2; i += TEXT_TPB) {
    if (i < n) {
      s_key[i] = fuse_order(s_sc[i]);
    } else {
      s_key[i] = 0u;
      s_id[i] = 0x7FFFFFFFFFFFFFFFll;
      s_sc[i] = 0.f;
    }
  }
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = tid; i < P2; i += TEXT_TPB) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t ka = s_key[i], kb = s_key[ixj];
          const int64_t ia = s_id[i], ib = s_id[ixj];
          const bool a_first = ka > kb || (ka == kb && ia < ib);
          const bool b_first = kb > ka || (ka == kb && ib < ia);
          if ((i & k) == 0 ? b_first : a_first) {
            const float fa = s_sc[i], fb = s_sc[ixj];
            s_key[i] = kb;
            s_id[i] = ib;
            s_sc[i] = fb;
            s_key[ixj] = ka;
            s_id[ixj] = ia;
            s_sc[ixj] = fa;
          }
        }
      }
    }
  __syncthreads();
  const int cnt = min(n, p.top_k);
  for (int j = tid; j < p.top_k; j += TEXT_TPB) {
    const int64_t at = (int64_t)b * p.top_k + j;
    p.out_ids[at] = j < cnt ? s_id[j] : 0;
    p.out_sc[at] = j < cnt ? s_sc[j] : 0.f;
  }
  if (tid == 0) p.out_cnt[b] = cnt;
}

// ---- host ------------------------------------------------------------------------------------------------------------


static int text_check_handle(const DeviceIndex* ix, bool need_text) {
  if (!ix) {
    set_error("Text search failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1) {
    set_error("Text search failed: the keyword index needs the whole index on the handle (opened with shard_count = %d): nRow, "
              "the average length and the hit counts are global figures; np_hip_index_set_text_shard and the sharded entries "
              "(np_hip_text_search_sharded, np_hip_search_hybrid_sharded) exchange them over a communicator",
              ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (need_text && !ix->text.present) {
    set_error("Text search failed: the handle has no keyword index (np_hip_index_set_text)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

// The checks of a batch of flat or tree queries against a vocabulary of n_terms; `check` is the query type's own
// (text_check_query, text_check_expr: np_text_plan.h).
template <class Q>
static int text_check_batch(int64_t n_terms, const Q* queries, int B, int top_k, int (*check)(const Q*, int32_t, int64_t, char*, size_t)) {
  const char* why = "";
  if (text_check_call(B, top_k, &why) != 0) {
    set_error("Text search failed: %s (B=%d top_k=%d)", why, B, top_k);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B > 0 && !queries) {
    set_error("Text search failed: NULL queries");
    return NP_ERR_INVALID_ARGUMENT;
  }
  char msg[320];
  for (int q = 0; q < B; ++q)
    if (check(&queries[q], q, n_terms, msg, sizeof msg) != 0) {
      set_error("Text search failed: %s", msg);
      return NP_ERR_INVALID_ARGUMENT;
    }
  return NP_OK;
}
// ... on a handle that holds the whole keyword index
static int text_check_queries(const DeviceIndex* ix, const np_text_query* queries, int B, int top_k) {
  NP_TRY(text_check_handle(ix, true));
  return text_check_batch(ix->text.n_terms, queries, B, top_k, text_check_query);
}
static int text_check_exprs(const DeviceIndex* ix, const np_text_expr* queries, int B, int top_k) {
  NP_TRY(text_check_handle(ix, true));
  return text_check_batch(ix->text.n_terms, queries, B, top_k, text_check_expr);
}

// A batch's queries as the kernels read them, one blob: q_phr | phr_tok | terms | mode | item_phr | nhit | idf, and behind them
// for a batch of tree queries (np_text_expr; `tree`): phr_hi | phr_slot | q_node | nodes | px_phr | px_at | pxhit.  A flat batch
// leaves the tree's fields at zero and nothing reads them.
struct TextProg {
  bool tree = false;
  int B = 0;
  int64_t n_phr = 0, n_tok = 0, n_items = 0;
  int64_t max_item_df = 0;
  int64_t per_query_extra = 0;   // arena bytes per query of a chunk beyond text_per_query (a tree query's prefix frequencies)
  size_t o_qphr = 0, o_ptok = 0, o_terms = 0, o_mode = 0, o_item = 0, o_nhit = 0, o_idf = 0, bytes = 0;
  std::vector<char> blob;
  std::vector<int64_t> phr_hit;   // nHit where the host knows it, -1 where the counting pass says
  // tree only.  A single-token phrase that ends in a prefix gets a slot: a per-document frequency array of its query, filled by
  // text_prefix_kernel, which also counts its nHit
  int slots = 0;             // frequency arrays a query of a chunk owns (the batch's maximum)
  int64_t stride = 0;        // entries of one
  int64_t n_px = 0;
  size_t o_phi = 0, o_slot = 0, o_qnode = 0, o_nodes = 0, o_pxphr = 0, o_pxat = 0, o_pxhit = 0;
  std::vector<int32_t> px_query;   // [n_px] the query of a prefix entry (entries ascend by query)
  int32_t* at32(size_t off) { return (int32_t*)(blob.data() + off); }
  void build(const DeviceIndex* ix, const np_text_query* qs, int B_) { build_phrases(ix, B_, [&](int q) { return qs[q]; }); }
  // the phrases of B_ queries; phrases_of(q): query q's terms, phrase offsets, phrase count and mode, as an np_text_query
  template <class F>
  void build_phrases(const DeviceIndex* ix, int B_, F phrases_of) {
    B = B_;
    for (int q = 0; q < B; ++q) {
      const np_text_query tq = phrases_of(q);
      n_phr += tq.n_phrases;
      n_tok += tq.phrase_offsets[tq.n_phrases];
    }
    phr_hit.assign((size_t)n_phr, 0);
    // sizes first: the items are known only after a walk
    o_qphr = 0;
    o_ptok = o_qphr + up256((size_t)(B + 1) * 4);
    o_terms = o_ptok + up256((size_t)(n_phr + 1) * 4);
    o_mode = o_terms + up256((size_t)std::max<int64_t>(n_tok, 1) * 4);
    o_item = o_mode + up256((size_t)std::max(B, 1) * 4);
    o_nhit = o_item + up256((size_t)std::max<int64_t>(n_phr, 1) * 4);
    o_idf = o_nhit + up256((size_t)std::max<int64_t>(n_phr, 1) * 8);
    bytes = o_idf + up256((size_t)std::max<int64_t>(n_phr, 1) * 8);
    blob.assign(bytes, 0);
    int32_t *qphr = at32(o_qphr), *ptok = at32(o_ptok), *terms = at32(o_terms), *mode = at32(o_mode), *item = at32(o_item);
    int64_t ph = 0, tk = 0;
    // (a rank of a sharded call that holds no keyword index still lays the programs out: the exchanges follow from them)
    const DeviceText& tx = ix->text;
    const std::vector<int64_t>& off = tx.h_post_off;   // the handle's own lists: the counting pass walks those
    for (int q = 0; q < B; ++q) {
      const np_text_query tq = phrases_of(q);
      qphr[q] = (int32_t)ph;
      mode[q] = tq.mode;
      for (int i = 0; i < tq.n_phrases; ++i, ++ph) {
        ptok[ph] = (int32_t)tk;
        const int tb = tq.phrase_offsets[i], te = tq.phrase_offsets[i + 1];
        bool known = true;
        for (int k = tb; k < te; ++k) {
          terms[tk++] = tq.terms[k];
          known = known && tq.terms[k] >= 0;
        }
        if (!known) {
          phr_hit[ph] = 0;
        } else if (te - tb == 1) {
          phr_hit[ph] = tx.present ? tx.df(tq.terms[tb]) : 0;   // (of the whole table, also on a shard)
        } else {
          phr_hit[ph] = -1;
          item[n_items++] = (int32_t)ph;
          if (tx.present) max_item_df = std::max(max_item_df, off[tq.terms[tb] + 1] - off[tq.terms[tb]]);
        }
      }
    }
    qphr[B] = (int32_t)ph;
    ptok[ph] = (int32_t)tk;
  }
  // tree queries: their phrases (planned and counted as a flat query's are), then the tree's part behind them
  void build_expr(const DeviceIndex* ix, const np_text_expr* es, int B_) {
    tree = true;
    build_phrases(ix, B_, [&](int q) { return np_text_query{es[q].terms, es[q].phrase_offsets, es[q].n_phrases, NP_TEXT_AND}; });
    int64_t n_nodes = 0;
    for (int q = 0; q < B; ++q) n_nodes += es[q].n_nodes;
    const size_t per_phr = up256((size_t)std::max<int64_t>(n_phr, 1) * 4);
    o_phi = bytes;
    o_slot = o_phi + per_phr;
    o_qnode = o_slot + per_phr;
    o_nodes = o_qnode + up256((size_t)(B + 1) * 4);
    o_pxphr = o_nodes + up256((size_t)std::max<int64_t>(n_nodes, 1) * 4);
    o_pxat = o_pxphr + per_phr;
    o_pxhit = o_pxat + per_phr;
    bytes = o_pxhit + 2 * per_phr;
    blob.resize(bytes, 0);
    int32_t *phi = at32(o_phi), *slot = at32(o_slot), *qnode = at32(o_qnode), *nodes = at32(o_nodes), *pxphr = at32(o_pxphr);
    int64_t ph = 0, nd = 0;
    for (int q = 0; q < B; ++q) {
      int used = 0;
      for (int i = 0; i < es[q].n_phrases; ++i, ++ph) {
        phi[ph] = es[q].prefix_hi[i];
        slot[ph] = -1;
        if (es[q].prefix_hi[i] != 0 && es[q].phrase_offsets[i + 1] - es[q].phrase_offsets[i] == 1) {
          slot[ph] = used++;
          pxphr[n_px++] = (int32_t)ph;
          px_query.push_back(q);
          phr_hit[(size_t)ph] = -1;   // the pre-pass of the query's chunk says
        }
      }
      slots = std::max(slots, used);
      qnode[q] = (int32_t)nd;
      for (int i = 0; i < es[q].n_nodes; ++i) nodes[nd++] = es[q].nodes[i].op | es[q].nodes[i].a << 8 | es[q].nodes[i].b << 16;
    }
    qnode[B] = (int32_t)nd;
    stride = (std::max<int64_t>(ix->n_docs, 1) + 63) / 64 * 64;
    per_query_extra = (int64_t)slots * stride * 4;   // (a multiple of 256)
  }
};

// bytes of the arena that scale with the chunk's queries -- one expression for the plan and for the carve-up
static int64_t text_per_query(const DeviceIndex* ix, int top_k, bool subsets) {
  const int64_t NW = std::max<int64_t>((ix->n_docs + 31) / 32, 1);
  return (int64_t)up256((size_t)top_k * 8) + (int64_t)up256((size_t)top_k * 4) + 8 + (subsets ? (int64_t)up256((size_t)NW * 4) : 0);
}
static int64_t text_n_slices(const DeviceIndex* ix) {
  return std::max<int64_t>(1, (ix->n_docs + NP_TEXT_SLICE_DOCS - 1) / NP_TEXT_SLICE_DOCS);
}
static int64_t text_fixed_bytes(const TextProg& prog) { return (int64_t)prog.bytes + 4096; }
static size_t text_arena_bytes(const DeviceIndex* ix, const TextPlan& plan, const TextProg& prog, int top_k, bool subsets) {
  const size_t pairs = (size_t)plan.queries * (size_t)plan.slices, keep = (size_t)text_slice_keep(top_k);
  return (size_t)text_fixed_bytes(prog) + (size_t)plan.queries * (size_t)(text_per_query(ix, top_k, subsets) + prog.per_query_extra) +
         up256(pairs * keep * 8) + up256(pairs * keep * 4) + up256(pairs * 4);
}
static int text_plan_for(const DeviceIndex* ix, int64_t user, const TextProg& prog, int B, int top_k, bool subsets, TextPlan* plan) {
  const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
  // (the three list arrays are each rounded up to 256 bytes: 768 more than the plan's pairs)
  if (!text_plan(budget, user + text_fixed_bytes(prog) + 1024, text_per_query(ix, top_k, subsets) + prog.per_query_extra,
                 text_n_slices(ix), B, ix->opts.max_batch, top_k, plan)) {
    set_error("Text search failed: one query over one slice of %lld documents does not fit the workspace budget of %lld bytes",
              (long long)NP_TEXT_SLICE_DOCS, (long long)budget);
    return NP_ERR_OUT_OF_MEMORY;
  }
  return NP_OK;
}

// The counting exchange of a sharded keyword search (np_dist_plan.h, dist_count_record): this rank's nHit of the counted phrases,
// its nRow and its status word go out, the sums over the healthy ranks come back.  A rank that cannot count (no keyword index,
// no workspace) sends zeros and its status.  Synchronises the stream: the idf is computed on the host.
struct TextCounts {
  const np_index* ix;
  np_comm* c;
  hipStream_t st;
  int64_t n_items;
  int rc;                 // this rank's local status as it goes out
  bool done = false;
  uint64_t failed = 0;    // the first non-zero status word among the gathered records
  int mismatch = 0, rank_a = 0, rank_b = 0;
  int run(const unsigned long long* d_nhit, int64_t n_rows, unsigned long long* h_sums) {
    const DistCountRec r = dist_count_record(n_items);
    const int G = c->nranks;
    NP_TRY(c->tx_cnt_local.reserve(r.bytes));
    NP_TRY(c->tx_cnt_all.reserve((size_t)G * r.bytes));
    char* loc = c->tx_cnt_local.as<char>();
    if (n_items > 0) {
      if (d_nhit && rc == NP_OK)
        NP_HIP(hipMemcpyAsync(loc, d_nhit, (size_t)n_items * 8, hipMemcpyDeviceToDevice, st));
      else
        NP_HIP(hipMemsetAsync(loc, 0, (size_t)n_items * 8, st));
    }
    NP_TRY(set_status_word(ix, (uint64_t*)(loc + r.o_rows), (uint64_t)n_rows, st));
    NP_TRY(set_status_word(ix, (uint64_t*)(loc + r.o_status), dist_status_word(c->rank, rc), st));
    const char* h_all = nullptr;
    NP_TRY(comm_all_gather(c, loc, c->tx_cnt_all.p, r.bytes, st, &h_all));
    std::vector<char> own;
    if (!h_all) {
      own.resize((size_t)G * r.bytes);
      NP_HIP(hipMemcpyAsync(own.data(), c->tx_cnt_all.p, own.size(), hipMemcpyDeviceToHost, st));
      NP_HIP(hipStreamSynchronize(st));
      h_all = own.data();
    }
    std::vector<uint64_t> sums((size_t)std::max<int64_t>(n_items, 1));
    int64_t rows = 0;
    mismatch = dist_sum_counts(h_all, r, G, sums.data(), &failed, &rows, &rank_a, &rank_b);
    if (h_sums)
      for (int64_t i = 0; i < n_items; ++i) h_sums[i] = (unsigned long long)sums[(size_t)i];
    done = true;
    return NP_OK;
  }
  // What every rank concludes alike from the gathered bytes: different tables are an argument error everywhere; with the
  // host-side check a failed rank ends the batch here.  (Otherwise the failure travels on to the merge.)
  bool all_leave() const { return done && (mismatch || (failed && c->host_check())); }
  int verdict() const {
    if (mismatch) {
      set_error("Text search failed: shards %d and %d report different nRow: every rank must be handed the same table "
                "(np_hip_index_set_text_shard)", rank_a, rank_b);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (failed && c->host_check()) {
      set_error("Search failed: shard %d failed with status %d; the batch was abandoned on every rank", dist_status_rank(failed),
                dist_status_code(failed));
      return NP_ERR_SEARCH;
    }
    return NP_OK;
  }
};

// The whole batch on device buffers.  `base`: the part of the arena this function carves (text_arena_bytes).  `pin`: pinned
// host staging of prog.bytes for the programs (the caller synchronises the stream before it reuses it), or NULL: pageable
// copies, and the stream is synchronised after the upload.  *visited (nullable): postings the scoring pass visited
// (synchronises).
// Sharded (counts != NULL): the hit counts of the counted phrases cross the ranks before the idf is computed, d_out_keys receives
// the f64 bits of the scores and the ids leave as global ids; otherwise both are NULL.
// Tree queries (prog.tree): the counting pass knows prefixes, every chunk of queries first fills the frequency arrays of its
// single-token prefix phrases and synchronises once for their nHit, and text_expr_kernel takes text_score_kernel's place.
// Sharded tree queries: text_prefix_count_kernel counts those phrases for the whole batch ahead of the chunk loop, in groups of
// bitmaps that fit the arena, so that their counts cross the ranks in the one counting exchange with the items'; the chunks
// then fill their frequency arrays without a synchronisation.  What crosses the ranks follows from the queries alone.
static int text_run(const DeviceIndex* ix, ContextUse& use, char* base, char* pin, const TextPlan& plan, TextProg& prog, int top_k,
                    const CallSubsets& sub, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, int64_t* visited,
                    unsigned long long* d_out_keys, TextCounts* counts) {
  hipStream_t st = use.stream;
  const DeviceText& tx = ix->text;
  const int B = prog.B;
  const bool tree = prog.tree;
  const bool subsets = sub.n > 0;
  const int64_t NW = std::max<int64_t>((ix->n_docs + 31) / 32, 1);
  const int Q = plan.queries;
  const int64_t S = plan.slices, n_slices = text_n_slices(ix);
  const int keep = (int)text_slice_keep(top_k);
  Carver carve{base};
  char* d_prog = carve.take(prog.bytes);
  unsigned long long* ctr = (unsigned long long*)carve.take(8);
  unsigned long long* best_keys = (unsigned long long*)carve.take((size_t)Q * up256((size_t)top_k * 8));
  int32_t* best_ids = (int32_t*)carve.take((size_t)Q * up256((size_t)top_k * 4));
  int32_t* best_cnt = (int32_t*)carve.take((size_t)Q * 4);
  int32_t* qrow = (int32_t*)carve.take((size_t)Q * 4);
  uint32_t* docbits = subsets ? (uint32_t*)carve.take((size_t)Q * up256((size_t)NW * 4)) : nullptr;
  unsigned long long* list_keys = (unsigned long long*)carve.take((size_t)Q * S * keep * 8);
  int32_t* list_ids = (int32_t*)carve.take((size_t)Q * S * keep * 4);
  int32_t* list_cnt = (int32_t*)carve.take((size_t)Q * S * 4);
  uint32_t* pfreq = prog.per_query_extra > 0 ? (uint32_t*)carve.take((size_t)Q * (size_t)prog.per_query_extra) : nullptr;
  // a prefix entry's frequency array: the place of its query in a chunk, then its slot
  for (int64_t i = 0; i < prog.n_px; ++i)
    prog.at32(prog.o_pxat)[i] = (prog.px_query[(size_t)i] % Q) * prog.slots + prog.at32(prog.o_slot)[prog.at32(prog.o_pxphr)[i]];
  const TextIxP tp{tx.post_off.get(), tx.post_doc.get(), tx.post_tf.get(), tx.post_first.get(), tx.pos.get(), tx.doc_len.get()};
  // the programs (everything before the hit counts), then the idf once every nHit is known
  char* src = prog.blob.data();
  if (pin) {
    memcpy(pin, src, prog.bytes);
    src = pin;
  }
  NP_HIP(hipMemcpyAsync(d_prog, src, prog.o_nhit, hipMemcpyHostToDevice, st));
  if (tree) {
    NP_HIP(hipMemcpyAsync(d_prog + prog.o_phi, src + prog.o_phi, prog.o_pxhit - prog.o_phi, hipMemcpyHostToDevice, st));
    NP_HIP(hipMemsetAsync(d_prog + prog.o_pxhit, 0, prog.bytes - prog.o_pxhit, st));
  }
  // the programs as the kernels take them
  auto d32 = [&](size_t off) { return (const int32_t*)(d_prog + off); };
  unsigned long long* d_nhit = (unsigned long long*)(d_prog + prog.o_nhit);
  unsigned long long* h_nhit = (unsigned long long*)(src + prog.o_nhit);
  // Over shards the single-token prefix phrases of a tree batch are counted here too, behind the items in the same vector:
  // their nHit must be summed over the ranks, and a collective cannot wait for a rank's own chunks
  const int64_t n_pre = counts && tree ? prog.n_px : 0;
  if (counts && counts->n_items != prog.n_items + n_pre) {   // (the record's size came from the queries alone: the same phrases)
    set_error("Text search failed: the counting exchange was sized for %lld phrases, the programs count %lld", (long long)counts->n_items,
              (long long)(prog.n_items + n_pre));
    return NP_ERR_SEARCH;
  }
  if (prog.n_items + n_pre > 0) {
    NP_HIP(hipMemsetAsync(d_nhit, 0, (size_t)(prog.n_items + n_pre) * 8, st));
    const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(NP_TEXT_HIT_BLOCKS, (prog.max_item_df + TEXT_TPB - 1) / TEXT_TPB));
    const auto hit_kernel = tree ? text_hit_kernel<true> : text_hit_kernel<false>;
    for (int64_t i0 = 0; i0 < prog.n_items; i0 += 65535) {   // (the items are a grid dimension)
      const TextHitP hp{tp, d32(prog.o_ptok), d32(prog.o_terms), tree ? d32(prog.o_phi) : nullptr, d32(prog.o_item) + i0, d_nhit + i0};
      hit_kernel<<<dim3(gx, (unsigned)std::min<int64_t>(65535, prog.n_items - i0)), TEXT_TPB, 0, st>>>(hp);
    }
    if (n_pre > 0 && ix->n_docs > 0) {
      // the bitmaps lie where the chunk loop's buffers will: nothing of those is live yet.  Groups of as many as fit
      const int64_t words = text_prefix_bitmap_bytes(ix->n_docs) / 4;
      const size_t arena_bytes = text_arena_bytes(ix, plan, prog, top_k, subsets);   // (what the caller reserved behind `base`)
      const int64_t group = text_prefix_group((int64_t)(base + arena_bytes - (char*)best_keys), ix->n_docs, n_pre);
      if (group < 1) {
        set_error("Text search failed: one bitmap of %lld documents does not fit the workspace", (long long)ix->n_docs);
        return NP_ERR_OUT_OF_MEMORY;
      }
      const int32_t* pxphr = prog.at32(prog.o_pxphr);
      for (int64_t x0 = 0; x0 < n_pre; x0 += group) {
        const int64_t xn = std::min(group, n_pre - x0);
        int64_t longest = 0;
        for (int64_t x = x0; x < x0 + xn; ++x) {
          const int32_t ph = pxphr[x], lo = prog.at32(prog.o_terms)[prog.at32(prog.o_ptok)[ph]], hi = prog.at32(prog.o_phi)[ph];
          longest = std::max(longest, tx.h_post_off[(size_t)hi] - tx.h_post_off[(size_t)lo]);
        }
        if (longest == 0) continue;   // no term of these ranges occurs on this shard: the counts stay 0
        NP_HIP(hipMemsetAsync(best_keys, 0, (size_t)xn * (size_t)words * 4, st));
        const unsigned gp = (unsigned)std::min<int64_t>(NP_TEXT_HIT_BLOCKS, (longest + TEXT_TPB - 1) / TEXT_TPB);
        const TextPrefixCountP cp{tp, d32(prog.o_ptok), d32(prog.o_terms), d32(prog.o_phi), d32(prog.o_pxphr) + x0, (uint32_t*)best_keys,
                                  words, d_nhit + prog.n_items + x0};
        text_prefix_count_kernel<<<dim3(gp, (unsigned)xn), TEXT_TPB, 0, st>>>(cp);
      }
    }
    NP_HIP(hipGetLastError());
    if (counts) {   // the shards' counts summed on the host, the same bytes on every rank
      NP_TRY(counts->run(d_nhit, tx.n_rows, h_nhit));
      NP_TRY(counts->verdict());
    } else {
      NP_HIP(hipMemcpyAsync(h_nhit, d_nhit, (size_t)prog.n_items * 8, hipMemcpyDeviceToHost, st));
      NP_HIP(hipStreamSynchronize(st));
    }
    const int32_t* item = (const int32_t*)(prog.blob.data() + prog.o_item);
    for (int64_t i = 0; i < prog.n_items; ++i) prog.phr_hit[(size_t)item[i]] = (int64_t)h_nhit[i];
    for (int64_t x = 0; x < n_pre; ++x) prog.phr_hit[(size_t)prog.at32(prog.o_pxphr)[x]] = (int64_t)h_nhit[prog.n_items + x];
  }
  double* h_idf = (double*)(src + prog.o_idf);
  // (nHit still -1: a single-token prefix phrase of a tree query.  Its idf is 0 here, no value bm25 can have, and is set by
  // its chunk's pre-pass below before any kernel reads it)
  for (int64_t ph = 0; ph < prog.n_phr; ++ph)
    h_idf[ph] = prog.phr_hit[(size_t)ph] < 0 ? 0.0 : text_idf(tx.n_rows, prog.phr_hit[(size_t)ph]);
  NP_HIP(hipMemcpyAsync(d_prog + prog.o_idf, h_idf, (size_t)std::max<int64_t>(prog.n_phr, 1) * 8, hipMemcpyHostToDevice, st));
  if (!pin) NP_HIP(hipStreamSynchronize(st));   // pageable sources: the copies complete before the blob goes out of scope
  if (visited) NP_HIP(hipMemsetAsync(ctr, 0, 8, st));
  const double avgdl = (double)tx.total_tokens / (double)tx.n_rows;
  int64_t px_visited = 0;   // postings the prefix pre-passes walk: counted on the host, with the scoring pass's in *visited
  // What the call fixes of the kernels' arguments, once; the loops below set the rest: q0, s0, qrow of the scoring kernels (the
  // last fields of TextScoreP) and Sn, n_prev and the outputs of the merge (0 and NULL here).  (The tree's part of a flat batch
  // is never read.)
  TextExprP xp{{tp, d32(prog.o_qphr), d32(prog.o_ptok), d32(prog.o_terms), (const double*)(d_prog + prog.o_idf), d32(prog.o_mode),
                ix->n_docs, avgdl, keep, docbits, NW, S, list_keys, list_ids, list_cnt, visited ? ctr : nullptr},
               d32(prog.o_phi), d32(prog.o_slot), d32(prog.o_qnode), d32(prog.o_nodes), pfreq, prog.stride, prog.slots};
  TextScoreP& sp = xp.s;
  TextMergeP mp{list_keys, list_ids, list_cnt, S, 0, keep, 0, best_keys, best_ids, best_cnt, top_k,
                nullptr, nullptr, nullptr, nullptr, counts ? ix->doc_begin : 0};
  for (int q0 = 0; q0 < B; q0 += Q) {
    const int Qn = std::min(Q, B - q0);
    bool chunk_subsets = subsets;
    if (subsets) {
      int64_t lo = 0, hi = sub.total;
      if (sub.h_off && sub.h_qsub) {   // only the ids this chunk's queries reference
        lo = sub.total;
        hi = 0;
        chunk_subsets = false;
        for (int b = 0; b < Qn; ++b) {
          const int32_t s = sub.h_qsub[q0 + b];
          if (s < 0) continue;
          chunk_subsets = true;
          if (sub.h_off[s + 1] == sub.h_off[s]) continue;
          lo = std::min(lo, sub.h_off[s]);
          hi = std::max(hi, sub.h_off[s + 1]);
        }
        if (hi < lo) lo = hi = 0;
      }
      if (chunk_subsets)
        NP_TRY(subset_doc_rows(ix, st, sub.d_ids, sub.d_off, sub.d_qsub + q0, sub.n, sub.total, lo, hi, Qn, NW, docbits, qrow));
    }
    if (tree) {   // the chunk's single-token prefix phrases: frequencies, nHit, idf
      int64_t x0 = 0, x1 = 0;
      while (x0 < prog.n_px && prog.px_query[(size_t)x0] < q0) ++x0;
      for (x1 = x0; x1 < prog.n_px && prog.px_query[(size_t)x1] < q0 + Qn; ++x1) {}
      if (x1 > x0 && ix->n_docs > 0) {
        NP_HIP(hipMemsetAsync(pfreq, 0, (size_t)Qn * (size_t)prog.per_query_extra, st));
        const int32_t* pxphr = prog.at32(prog.o_pxphr);
        int64_t longest = 0;
        for (int64_t x = x0; x < x1; ++x) {
          const int32_t ph = pxphr[x], lo = prog.at32(prog.o_terms)[prog.at32(prog.o_ptok)[ph]], hi = prog.at32(prog.o_phi)[ph];
          longest = std::max(longest, tx.h_post_off[(size_t)hi] - tx.h_post_off[(size_t)lo]);
          px_visited += tx.h_post_off[(size_t)hi] - tx.h_post_off[(size_t)lo];
        }
        const unsigned gx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(NP_TEXT_HIT_BLOCKS, (longest + TEXT_TPB - 1) / TEXT_TPB));
        for (int64_t i0 = x0; i0 < x1; i0 += 65535) {   // (the entries are a grid dimension)
          const TextPrefixP pp{tp, d32(prog.o_ptok), d32(prog.o_terms), d32(prog.o_phi), d32(prog.o_pxphr) + i0, d32(prog.o_pxat) + i0,
                               pfreq, prog.stride, (unsigned long long*)(d_prog + prog.o_pxhit)};
          text_prefix_kernel<<<dim3(gx, (unsigned)std::min<int64_t>(65535, x1 - i0)), TEXT_TPB, 0, st>>>(pp);
        }
        NP_HIP(hipGetLastError());
        if (!counts) {   // (over shards the counting pre-pass has summed these counts: the chunk's own is not used)
          const int32_t p0 = prog.at32(prog.o_qphr)[q0], p1 = prog.at32(prog.o_qphr)[q0 + Qn];
          unsigned long long* h_px = (unsigned long long*)(src + prog.o_pxhit);
          NP_HIP(hipMemcpyAsync(h_px + p0, d_prog + prog.o_pxhit + (size_t)p0 * 8, (size_t)(p1 - p0) * 8, hipMemcpyDeviceToHost, st));
          NP_HIP(hipStreamSynchronize(st));
          for (int64_t x = x0; x < x1; ++x) {
            const int32_t ph = pxphr[x];
            prog.phr_hit[(size_t)ph] = (int64_t)h_px[ph];
            h_idf[ph] = text_idf(tx.n_rows, prog.phr_hit[(size_t)ph]);
          }
          NP_HIP(hipMemcpyAsync(d_prog + prog.o_idf + (size_t)p0 * 8, h_idf + p0, (size_t)(p1 - p0) * 8, hipMemcpyHostToDevice, st));
          if (!pin) NP_HIP(hipStreamSynchronize(st));   // a pageable source: the copy completes before the blob goes out of scope
        }
      }
    }
    sp.q0 = q0;
    sp.qrow = chunk_subsets ? qrow : nullptr;
    mp.out_ids = d_out_ids + (int64_t)q0 * top_k;
    mp.out_scores = d_out_scores + (int64_t)q0 * top_k;
    mp.out_counts = d_out_counts + q0;
    mp.out_keys = d_out_keys ? d_out_keys + (int64_t)q0 * top_k : nullptr;
    for (int64_t s0 = 0; s0 < n_slices; s0 += S) {
      const int64_t Sn = std::min(S, n_slices - s0);
      sp.s0 = s0;
      if (ix->n_docs > 0 && tree)
        text_expr_kernel<<<dim3((unsigned)Sn, (unsigned)Qn), TEXT_TPB, 0, st>>>(xp);
      else if (ix->n_docs > 0)
        text_score_kernel<<<dim3((unsigned)Sn, (unsigned)Qn), TEXT_TPB, 0, st>>>(sp);
      mp.Sn = ix->n_docs > 0 ? Sn : 0;
      mp.n_prev = s0 > 0 ? 1 : 0;
      text_merge_kernel<<<(unsigned)Qn, TEXT_TPB, 0, st>>>(mp);
      NP_HIP(hipGetLastError());
    }
  }
  if (visited) {
    unsigned long long h = 0;
    NP_HIP(hipMemcpyAsync(&h, ctr, 8, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    *visited = (int64_t)h + px_visited;
  }
  return NP_OK;
}

// np_hip_text_search and np_hip_text_search_filtered: the subsets come as a host CSR, or (filters != NULL) are evaluated on
// the call's context into a CSR that stays on the device; query_subset is the query map of either.  exprs != NULL: the _expr
// forms, tree queries in place of `queries` (a NULL batch gets the flat form's checks: they say so)
static int text_host(const np_index* ix, const np_text_query* queries, const np_text_expr* exprs, int32_t B, int32_t top_k,
                     const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets, const int32_t* query_subset,
                     const np_filter* filters, int64_t* out_ids, float* out_scores, int32_t* out_counts, np_stats* stats) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  if (stats) memset(stats, 0, sizeof *stats);
  NP_TRY(exprs ? text_check_exprs(ix, exprs, B, top_k) : text_check_queries(ix, queries, B, top_k));
  if (filters)
    NP_TRY(filter_check_call(ix, filters, (int32_t)n_subsets, query_subset, B, true));
  else
    NP_TRY(check_subsets(subset_ids, subset_offsets, n_subsets, query_subset, query_subset, B));
  if (B == 0) return NP_OK;
  if (!out_ids || !out_scores || !out_counts) {
    set_error("Text search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const auto t0 = std::chrono::steady_clock::now();
  TextProg prog;
  if (exprs) prog.build_expr(ix, exprs, B); else prog.build(ix, queries, B);
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  HostScope scope;
  NP_TRY(scope.resolve(ix, use, subset_ids, subset_offsets, n_subsets, query_subset, filters, B));
  ResultStage res(B, top_k);
  const size_t user = scope.stage_bytes() + res.bytes();
  TextPlan plan;
  NP_TRY(text_plan_for(ix, (int64_t)user + scope.budget_extra(), prog, B, top_k, scope.any, &plan));
  NP_TRY(use.arena().reserve(user + text_arena_bytes(ix, plan, prog, top_k, scope.any)));
  void* pin = nullptr;   // the results, the programs behind them
  NP_TRY(use.pin(res.bytes() + prog.bytes, &pin));
  Carver carve{use.arena().as<char>()};
  CallSubsets sub;
  NP_TRY(scope.place(carve, st, &sub));
  res.carve(carve);
  int64_t visited = 0;
  NP_TRY(text_run(ix, use, carve.at, (char*)pin + res.bytes(), plan, prog, top_k, sub, res.d_ids, res.d_sc, res.d_cnt,
                  stats ? &visited : nullptr, nullptr, nullptr));
  NP_TRY(res.fetch(pin, st));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_counts);
  if (stats) {
    stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->n_queries = B;
    stats->n_ivf_ids = visited;
  }
  return NP_OK;
}

// a hybrid result over document shards: a list that came back abandoned (count -1: a peer failed) abandons the fused result too
__global__ void hybrid_abandon_kernel(const int32_t* __restrict__ sem_cnt, const int32_t* __restrict__ kw_cnt, int B,
                                      int32_t* __restrict__ out_cnt) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && (sem_cnt[b] < 0 || kw_cnt[b] < 0)) out_cnt[b] = NP_COUNT_ABANDONED;
}

static int fuse_launch(hipStream_t st, int mode, float alpha, int top_k, int B, const int64_t* sem_ids, const float* sem_sc,
                       const int32_t* sem_cnt, int sem_stride, const int64_t* kw_ids, const float* kw_sc, const int32_t* kw_cnt,
                       int kw_stride, int64_t* out_ids, float* out_sc, int32_t* out_cnt) {
  const FuseP p{mode, alpha, top_k, sem_ids, sem_sc, sem_cnt, sem_stride, kw_ids, kw_sc, kw_cnt, kw_stride, out_ids, out_sc, out_cnt};
  fuse_kernel<<<(unsigned)B, TEXT_TPB, 0, st>>>(p);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

static int fuse_check(int mode, float alpha, int top_k, int B, int sem_stride, int kw_stride) {
  const char* why = "";
  if (fuse_check_call(mode, alpha, top_k, B, sem_stride, kw_stride, &why) != 0) {
    set_error("Fusion failed: %s (mode=%d alpha=%g top_k=%d strides %d, %d)", why, mode, (double)alpha, top_k, sem_stride, kw_stride);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}


// ---- the keyword search over document shards (np_hip_text_search_sharded) ---------------------------------------------------

// the checks of a sharded keyword call that depend on its arguments alone: every rank passes or fails them alike, so a failure
// returns before the first collective.  (The vocabulary check needs the handle's index: a rank that fails it fails locally.)
static int text_check_sharded_args(const np_index* ix, np_comm* c, const np_text_query* queries, const np_text_expr* exprs, int B, int top_k,
                                   const void* out_ids, const void* out_scores, const void* out_counts, void* stream) {
  if (!ix || !c || !stream) {
    set_error("Text search failed: NULL index / communicator / stream (the collectives need the caller's stream)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (exprs)
    NP_TRY(text_check_batch((int64_t)1 << 31, exprs, B, top_k, text_check_expr));
  else
    NP_TRY(text_check_batch((int64_t)1 << 31, queries, B, top_k, text_check_query));
  if (B > 0 && (!out_ids || !out_scores || !out_counts)) {
    set_error("Text search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

// phrases of several tokens, all known: the ones the counting pass counts.  Follows from the queries alone, so every rank runs the
// counting exchange or none does.
static int64_t text_counted_phrases(const np_text_query* queries, int B) {
  int64_t n = 0;
  for (int q = 0; q < B; ++q)
    for (int i = 0; i < queries[q].n_phrases; ++i) {
      const int tb = queries[q].phrase_offsets[i], te = queries[q].phrase_offsets[i + 1];
      bool known = true;
      for (int k = tb; k < te; ++k) known = known && queries[q].terms[k] >= 0;
      n += known && te - tb > 1 ? 1 : 0;
    }
  return n;
}

// The sharded keyword pass; the caller holds c->mu and has checked the arguments.  `exprs` != NULL: tree queries in place of
// `queries`.  `sub`: the scope on the device (global ids; ids of other shards are ignored, the rest rebased).  rc0 / msg0: a local failure the caller already met.
//   [a batch with a counted phrase]  text_hit_kernel (and, for the single-token prefix phrases of tree queries,
//   text_prefix_count_kernel) on the shard -> all-gather of nhit | nRow | status -> sums on the host
//   local scoring with the global idf and average length -> the shard's top-k as f64 keys and global ids
//   per exchange (np_dist_plan.h cuts the batch by B and top_k alone): all-gather of keys | ids | counts | status,
//   text_rank_merge_kernel into the caller's buffers
static int text_sharded_locked(const np_index* ix, np_comm* c, const np_text_query* queries, const np_text_expr* exprs, int B, int top_k,
                               const CallSubsets& sub, int rc0, const char* msg0, int64_t* d_out_ids, float* d_out_scores,
                               int32_t* d_out_counts, hipStream_t st) {
  DeviceGuard g(ix->device);
  const int G = c->nranks;
  const bool host_check = c->host_check();
  const int Bx = dist_text_exchange_queries(B, top_k), n_ex = dist_text_exchanges(B, top_k);
  const DistTextRec rmax = dist_text_record(Bx, top_k);
  const size_t n_all = (size_t)B * top_k;
  // the communicator's own buffers: fatal before the first collective, as in the semantic pass
  NP_TRY(c->tx_local.reserve(rmax.bytes));
  NP_TRY(c->tx_all.reserve((size_t)G * rmax.bytes));
  if (n_ex > 1) NP_TRY(c->tx_src.reserve(n_all * 16 + (size_t)B * 4));
  char* loc = c->tx_local.as<char>();
  // the shard's lists of the whole batch: straight in the record where one exchange carries the batch
  unsigned long long* l_keys = (unsigned long long*)(n_ex > 1 ? c->tx_src.as<char>() : loc);
  int64_t* l_ids = (int64_t*)(n_ex > 1 ? c->tx_src.as<char>() + n_all * 8 : loc + rmax.o_ids);
  int32_t* l_cnt = (int32_t*)(n_ex > 1 ? c->tx_src.as<char>() + n_all * 16 : loc + rmax.o_counts);
  int rc = rc0;
  std::string rc_msg = rc0 != NP_OK && msg0 ? msg0 : "";
  auto local = [&](int r) {
    if (r != NP_OK && rc == NP_OK) {
      rc = r;
      rc_msg = np_hip_last_error();
    }
    return r == NP_OK;
  };
  auto finish = [&](int r) {
    if (r != NP_OK && !rc_msg.empty()) set_error("%s", rc_msg.c_str());
    return r;
  };
  auto peer_failed = [&](uint64_t w) {
    set_error("Search failed: shard %d failed with status %d; the batch was abandoned on every rank", dist_status_rank(w),
              dist_status_code(w));
    return (int)NP_ERR_SEARCH;
  };
  if (rc == NP_OK && !ix->text.present) {
    set_error("Text search failed: the handle has no keyword index (np_hip_index_set_text_shard)");
    local(NP_ERR_INVALID_ARGUMENT);
  }
  char msg[320];
  for (int q = 0; rc == NP_OK && q < B; ++q)
    if ((exprs ? text_check_expr(&exprs[q], q, ix->text.n_terms, msg, sizeof msg)
               : text_check_query(&queries[q], q, ix->text.n_terms, msg, sizeof msg)) != 0) {
      set_error("Text search failed: %s", msg);
      local(NP_ERR_INVALID_ARGUMENT);
    }
  TextCounts counts{ix, c, st, exprs ? text_counted_expr_phrases(exprs, B) : text_counted_phrases(queries, B), rc};
  {
    TextProg prog;
    TextPlan plan;
    ContextUse use;
    if (rc == NP_OK) {
      if (exprs) prog.build_expr(ix, exprs, B); else prog.build(ix, queries, B);
      local(text_plan_for(ix, 0, prog, B, top_k, sub.n > 0, &plan));
    }
    if (rc == NP_OK) local(use.begin(ix, st));
    if (rc == NP_OK) local(use.arena().reserve(text_arena_bytes(ix, plan, prog, top_k, sub.n > 0)));
    counts.rc = rc;
    if (rc == NP_OK) {
      // (the f32 scores of the local lists land in the caller's score buffer: the merge below overwrites it)
      const int r = text_run(ix, use, use.arena().as<char>(), nullptr, plan, prog, top_k, sub, l_ids, d_out_scores, l_cnt, nullptr, l_keys,
                             &counts);
      if (r != NP_OK && counts.all_leave()) return r;   // every rank read the same bytes and leaves here
      local(r);
    }
    if (counts.n_items > 0 && !counts.done) {   // this rank could not count: it still takes part, with zeros and its status
      counts.rc = rc;
      NP_TRY(counts.run(nullptr, 0, nullptr));
      if (counts.all_leave()) return rc != NP_OK ? finish(rc) : counts.verdict();
    }
  }
  for (int e = 0; e < n_ex; ++e) {
    const int q0 = e * Bx, Bl = std::min(Bx, B - q0);
    const DistTextRec r = dist_text_record(Bl, top_k);
    const size_t n = (size_t)Bl * top_k;
    if (rc != NP_OK) {
      NP_HIP(hipMemsetAsync(loc, 0, r.o_status, st));   // counts 0
    } else if (n_ex > 1) {
      NP_HIP(hipMemcpyAsync(loc, l_keys + (size_t)q0 * top_k, n * 8, hipMemcpyDeviceToDevice, st));
      NP_HIP(hipMemcpyAsync(loc + r.o_ids, l_ids + (size_t)q0 * top_k, n * 8, hipMemcpyDeviceToDevice, st));
      NP_HIP(hipMemcpyAsync(loc + r.o_counts, l_cnt + q0, (size_t)Bl * 4, hipMemcpyDeviceToDevice, st));
    }
    NP_TRY(set_status_word(ix, (uint64_t*)(loc + r.o_status), dist_status_word(c->rank, rc), st));
    const char* h_all = nullptr;
    NP_TRY(comm_all_gather(c, loc, c->tx_all.p, r.bytes, st, &h_all));
    // (a rank that reports the failure by its return code must not also leave the word behind for the next healthy batch)
    const TextRankMergeP mp{c->tx_all.as<char>(), (int64_t)r.bytes, (int64_t)r.o_ids, (int64_t)r.o_counts, (int64_t)r.o_status, G, top_k,
                            d_out_ids + (size_t)q0 * top_k, d_out_scores + (size_t)q0 * top_k, d_out_counts + q0,
                            (rc == NP_OK && !host_check) ? (unsigned long long*)c->h_status : nullptr};
    text_rank_merge_kernel<<<(unsigned)Bl, TEXT_TPB, 0, st>>>(mp);
    NP_HIP(hipGetLastError());
    if (host_check && h_all) {
      const uint64_t w = dist_first_failure(h_all, r.bytes, r.o_status, G);
      if (w) return rc != NP_OK ? finish(rc) : peer_failed(w);
    }
  }
  return finish(rc);
}

}  // namespace np

using namespace np;

extern "C" {

// np_hip_index_set_text, and np_hip_index_set_text_shard on a sharded handle (slice): the arrays describe the whole table either
// way; a slice keeps the postings, positions and lengths of its own documents [doc_begin, doc_begin + n_docs) under shard-local
// ids, and the whole table's nRow, token count and document frequencies on the host.
static int set_text_impl(np_index* ix, const np_text_index* text, bool slice) {
  DeviceGuard g(ix->device);
  DeviceText fresh;
  size_t bytes = 0;
  char why[240];
  const int64_t n_table = slice ? ix->N_total : ix->n_docs;   // documents the table may name
  if (text && text_check_index(text, n_table, why, sizeof why) != 0) {
    set_error("set_text: %s", why);
    return NP_ERR_INVALID_ARGUMENT;
  }
  // NULL, or an index without instances and rows, drops what the handle had
  if (text && !((text->n_terms == 0 || text->term_offsets[text->n_terms] == 0) && text->n_rows == 0)) {
    // postings and document lengths, derived on the host; the new index is built beside the old one and swapped in whole
    const int64_t n_terms = text->n_terms, n_inst = n_terms > 0 ? text->term_offsets[n_terms] : 0;
    const int64_t d_lo = slice ? ix->doc_begin : 0, d_hi = d_lo + ix->n_docs;
    std::vector<int64_t> post_off((size_t)n_terms + 1, 0), post_first, df;
    std::vector<int32_t> post_doc, post_tf, doc_len((size_t)std::max<int64_t>(ix->n_docs, 1), 0), own_pos;
    if (slice) df.assign((size_t)n_terms, 0);
    for (int64_t k = 0; k < n_terms; ++k) {
      int64_t prev = -1;
      bool first = true;
      for (int64_t i = text->term_offsets[k]; i < text->term_offsets[k + 1]; ++i) {
        const int64_t gd = text->inst_doc[i];
        if (slice && gd != prev) ++df[(size_t)k];
        prev = gd;
        if (gd < d_lo || gd >= d_hi) continue;
        const int32_t d = (int32_t)(gd - d_lo);
        if (first || post_doc.back() != d) {
          post_doc.push_back(d);
          post_tf.push_back(0);
          post_first.push_back(slice ? (int64_t)own_pos.size() : i);
          first = false;
        }
        if (slice) own_pos.push_back(text->inst_pos[i]);
        ++post_tf.back();
        ++doc_len[(size_t)d];
      }
      post_off[(size_t)k + 1] = (int64_t)post_doc.size();
    }
    const size_t n_post = post_doc.size();
    const int64_t n_own = slice ? (int64_t)own_pos.size() : n_inst;
    const int32_t* pos_src = slice ? own_pos.data() : text->inst_pos;
    NP_TRY(fresh.post_off.alloc((size_t)n_terms + 1, &bytes));
    NP_TRY(fresh.post_doc.alloc(n_post, &bytes));
    NP_TRY(fresh.post_tf.alloc(n_post, &bytes));
    NP_TRY(fresh.post_first.alloc(n_post, &bytes));
    NP_TRY(fresh.pos.alloc((size_t)n_own, &bytes));
    NP_TRY(fresh.doc_len.alloc(doc_len.size(), &bytes));
    NP_HIP(hipMemcpy(fresh.post_off.get(), post_off.data(), post_off.size() * 8, hipMemcpyHostToDevice));
    if (n_post > 0) {
      NP_HIP(hipMemcpy(fresh.post_doc.get(), post_doc.data(), n_post * 4, hipMemcpyHostToDevice));
      NP_HIP(hipMemcpy(fresh.post_tf.get(), post_tf.data(), n_post * 4, hipMemcpyHostToDevice));
      NP_HIP(hipMemcpy(fresh.post_first.get(), post_first.data(), n_post * 8, hipMemcpyHostToDevice));
      NP_HIP(hipMemcpy(fresh.pos.get(), pos_src, (size_t)n_own * 4, hipMemcpyHostToDevice));
    }
    NP_HIP(hipMemcpy(fresh.doc_len.get(), doc_len.data(), doc_len.size() * 4, hipMemcpyHostToDevice));
    fresh.n_terms = n_terms;
    fresh.n_post = (int64_t)n_post;
    fresh.n_inst = n_own;
    fresh.n_rows = text->n_rows;
    fresh.total_tokens = n_inst;   // (the whole table's, also on a slice)
    fresh.h_post_off = std::move(post_off);
    fresh.h_df = std::move(df);
    fresh.slice = slice;
    fresh.present = true;
  }
  ix->text = std::move(fresh);
  ix->device_bytes = ix->device_bytes - ix->text_bytes + bytes;
  ix->text_bytes = bytes;
  return NP_OK;
}

int np_hip_index_set_text(np_index* ix, const np_text_index* text) {
  clear_error();
  NP_TRY(text_check_handle(ix, false));
  return set_text_impl(ix, text, false);
}

int np_hip_index_set_text_shard(np_index* ix, const np_text_index* text) {
  clear_error();
  if (!ix) {
    set_error("Text search failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return set_text_impl(ix, text, ix->opts.shard_count > 1);
}

int np_hip_text_search(const np_index* ix, const np_text_query* queries, int32_t B, int32_t top_k, const int64_t* subset_ids,
                       const int64_t* subset_offsets, int64_t n_subsets, const int32_t* query_subset, int64_t* out_ids,
                       float* out_scores, int32_t* out_counts, np_stats* stats) {
  return text_host(ix, queries, nullptr, B, top_k, subset_ids, subset_offsets, n_subsets, query_subset, nullptr, out_ids, out_scores,
                   out_counts, stats);
}

int np_hip_text_search_expr(const np_index* ix, const np_text_expr* queries, int32_t B, int32_t top_k, const int64_t* subset_ids,
                            const int64_t* subset_offsets, int64_t n_subsets, const int32_t* query_subset, int64_t* out_ids,
                            float* out_scores, int32_t* out_counts, np_stats* stats) {
  return text_host(ix, nullptr, queries, B, top_k, subset_ids, subset_offsets, n_subsets, query_subset, nullptr,
                   out_ids, out_scores, out_counts, stats);
}

int np_hip_text_search_expr_filtered(const np_index* ix, const np_text_expr* queries, int32_t B, int32_t top_k,
                                     const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int64_t* out_ids,
                                     float* out_scores, int32_t* out_counts, np_stats* stats) {
  static const np_filter none{};
  return text_host(ix, nullptr, queries, B, top_k, nullptr, nullptr, n_filters, query_filter,
                   filters ? filters : &none, out_ids, out_scores, out_counts, stats);
}

int np_hip_text_search_filtered(const np_index* ix, const np_text_query* queries, int32_t B, int32_t top_k,
                                const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int64_t* out_ids,
                                float* out_scores, int32_t* out_counts, np_stats* stats) {
  static const np_filter none{};   // n_filters == 0: nothing to check or evaluate, but still the filtered call's checks
  return text_host(ix, queries, nullptr, B, top_k, nullptr, nullptr, n_filters, query_filter, filters ? filters : &none, out_ids,
                   out_scores, out_counts, stats);
}

// np_hip_text_search_device, and with exprs != NULL np_hip_text_search_expr_device (a NULL batch gets the flat form's checks: they
// say so)
static int text_device(const np_index* ix, const np_text_query* queries, const np_text_expr* exprs, int32_t B, int32_t top_k,
                       const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                       int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                       int32_t* d_out_counts, void* stream) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  NP_TRY(exprs ? text_check_exprs(ix, exprs, B, top_k) : text_check_queries(ix, queries, B, top_k));
  NP_TRY(check_device_subsets(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, B));
  if (B == 0) return NP_OK;
  if (!d_out_ids || !d_out_scores || !d_out_counts) {
    set_error("Text search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const CallSubsets sub = CallSubsets::device(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset);
  TextProg prog;
  if (exprs) prog.build_expr(ix, exprs, B); else prog.build(ix, queries, B);
  DeviceGuard g(ix->device);
  TextPlan plan;
  NP_TRY(text_plan_for(ix, 0, prog, B, top_k, sub.n > 0, &plan));
  ContextUse use;
  NP_TRY(use.begin(ix, stream));
  NP_TRY(use.arena().reserve(text_arena_bytes(ix, plan, prog, top_k, sub.n > 0)));
  return text_run(ix, use, use.arena().as<char>(), nullptr, plan, prog, top_k, sub, d_out_ids, d_out_scores, d_out_counts, nullptr, nullptr,
                  nullptr);
}

int np_hip_text_search_device(const np_index* ix, const np_text_query* queries, int32_t B, int32_t top_k,
                              const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                              int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                              int32_t* d_out_counts, void* stream) {
  return text_device(ix, queries, nullptr, B, top_k, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset,
                     d_out_ids, d_out_scores, d_out_counts, stream);
}

int np_hip_text_search_expr_device(const np_index* ix, const np_text_expr* queries, int32_t B, int32_t top_k,
                                   const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                   int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                                   int32_t* d_out_counts, void* stream) {
  return text_device(ix, nullptr, queries, B, top_k, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset,
                     d_out_ids, d_out_scores, d_out_counts, stream);
}

int np_hip_fuse_device(const np_index* ix, int32_t mode, float alpha, int32_t top_k, int32_t B, const int64_t* d_sem_ids,
                       const float* d_sem_scores, const int32_t* d_sem_counts, int32_t sem_stride, const int64_t* d_kw_ids,
                       const float* d_kw_scores, const int32_t* d_kw_counts, int32_t kw_stride, int64_t* d_out_ids,
                       float* d_out_scores, int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(fuse_check(mode, alpha, top_k, B, sem_stride, kw_stride));
  if (B == 0) return NP_OK;
  if (!d_sem_ids || !d_sem_counts || !d_kw_ids || !d_kw_counts || !d_out_ids || !d_out_scores || !d_out_counts ||
      (mode == NP_FUSE_RELATIVE_SCORE && (!d_sem_scores || !d_kw_scores))) {
    set_error("Fusion failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!ix)   // the current device: the kernel needs no scratch
    return fuse_launch((hipStream_t)stream, mode, alpha, top_k, B, d_sem_ids, d_sem_scores, d_sem_counts, sem_stride, d_kw_ids,
                       d_kw_scores, d_kw_counts, kw_stride, d_out_ids, d_out_scores, d_out_counts);
  DeviceGuard g(ix->device);
  ContextUse use;   // (a context's stream where `stream` is NULL)
  NP_TRY(use.begin(ix, stream));
  return fuse_launch(use.stream, mode, alpha, top_k, B, d_sem_ids, d_sem_scores, d_sem_counts, sem_stride, d_kw_ids, d_kw_scores,
                     d_kw_counts, kw_stride, d_out_ids, d_out_scores, d_out_counts);
}

int np_hip_fuse(const np_index* ix, int32_t mode, float alpha, int32_t top_k, int32_t B, const int64_t* sem_ids,
                const float* sem_scores, const int32_t* sem_counts, int32_t sem_stride, const int64_t* kw_ids,
                const float* kw_scores, const int32_t* kw_counts, int32_t kw_stride, int64_t* out_ids, float* out_scores,
                int32_t* out_counts) {
  clear_error();
  NP_TRY(fuse_check(mode, alpha, top_k, B, sem_stride, kw_stride));
  if (B == 0) return NP_OK;
  const bool rel = mode == NP_FUSE_RELATIVE_SCORE;
  if (!sem_counts || !kw_counts || !out_ids || !out_scores || !out_counts || (sem_stride > 0 && (!sem_ids || (rel && !sem_scores))) ||
      (kw_stride > 0 && (!kw_ids || (rel && !kw_scores)))) {
    set_error("Fusion failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int b = 0; b < B; ++b)
    if (sem_counts[b] < 0 || sem_counts[b] > sem_stride || kw_counts[b] < 0 || kw_counts[b] > kw_stride) {
      set_error("Fusion failed: the counts of query %d (%d, %d) are outside their strides (%d, %d)", b, sem_counts[b], kw_counts[b],
                sem_stride, kw_stride);
      return NP_ERR_INVALID_ARGUMENT;
    }
  const size_t n_s = (size_t)B * sem_stride, n_k = (size_t)B * kw_stride;
  const size_t b_si = up256(n_s * 8), b_ss = up256(n_s * 4), b_ki = up256(n_k * 8), b_ks = up256(n_k * 4), b_c = up256((size_t)B * 4);
  ResultStage res(B, top_k);
  const size_t dev_bytes = b_si + b_ss + b_ki + b_ks + 2 * b_c + res.bytes();
  // with a handle: its device, a context's stream, arena and pinned staging; without: the current device, the call's own
  int device = 0;
  if (ix) device = ix->device; else (void)hipGetDevice(&device);
  DeviceGuard g(device);
  ContextUse use;
  DevPtr<char> own;
  std::vector<char> own_host;
  hipStream_t st = nullptr;
  void* pin = nullptr;
  Carver carve{nullptr};
  if (ix) {
    NP_TRY(use.begin(ix, nullptr));
    st = use.stream;
    NP_TRY(use.arena().reserve(dev_bytes));
    NP_TRY(use.pin(res.bytes(), &pin));
    carve.at = use.arena().as<char>();
  } else {
    NP_TRY(own.alloc(dev_bytes));
    own_host.resize(res.bytes());
    pin = own_host.data();
    carve.at = own.get();
  }
  int64_t* d_si = (int64_t*)carve.take(b_si);
  float* d_ss = (float*)carve.take(b_ss);
  int64_t* d_ki = (int64_t*)carve.take(b_ki);
  float* d_ks = (float*)carve.take(b_ks);
  int32_t *d_sc = (int32_t*)carve.take(b_c), *d_kc = (int32_t*)carve.take(b_c);
  res.carve(carve);
  // pageable sources: the copies complete before the call returns (it synchronises below)
  if (n_s > 0) NP_HIP(hipMemcpyAsync(d_si, sem_ids, n_s * 8, hipMemcpyHostToDevice, st));
  if (n_s > 0 && sem_scores) NP_HIP(hipMemcpyAsync(d_ss, sem_scores, n_s * 4, hipMemcpyHostToDevice, st));
  if (n_k > 0) NP_HIP(hipMemcpyAsync(d_ki, kw_ids, n_k * 8, hipMemcpyHostToDevice, st));
  if (n_k > 0 && kw_scores) NP_HIP(hipMemcpyAsync(d_ks, kw_scores, n_k * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_sc, sem_counts, (size_t)B * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_kc, kw_counts, (size_t)B * 4, hipMemcpyHostToDevice, st));
  NP_TRY(fuse_launch(st, mode, alpha, top_k, B, d_si, sem_scores ? d_ss : nullptr, d_sc, sem_stride, d_ki, kw_scores ? d_ks : nullptr,
                     d_kc, kw_stride, res.d_ids, res.d_sc, res.d_cnt));
  NP_TRY(res.fetch(pin, st));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_counts);
  return NP_OK;
}

// The hybrid request.  grp == NULL: np_hip_search_hybrid, fused to params->top_k.  Otherwise np_hip_search_hybrid_grouped: fused
// to grp->pool_k into a list that stays on the device, then collapsed to params->top_k groups (np_group.hip) on the same stream.
static int hybrid_host(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                       const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k, float alpha,
                       int32_t fusion, const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                       const int32_t* query_subset, const np_filter* filters, int32_t n_filters, int64_t* out_ids,
                       float* out_scores, int32_t* out_counts, np_stats* stats, const GroupCall* grp,
                       const np_text_expr* text_exprs = nullptr) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  if (stats) memset(stats, 0, sizeof *stats);
  if (!params) {
    set_error("Search failed: NULL index or params");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(text_exprs ? text_check_exprs(ix, text_exprs, B, fetch_k) : text_check_queries(ix, text_queries, B, fetch_k));
  NP_TRY(fuse_check(fusion, alpha, grp ? grp->pool_k : params->top_k, B, fetch_k, fetch_k));
  if (grp) NP_TRY(collapse_check(ix, params->top_k, grp->group_size, B, grp->pool_k));
  if (grp && B > 0 && (!grp->out_group || !grp->out_members || !grp->out_total)) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (filters) n_subsets = n_filters;
  if (filters)
    NP_TRY(filter_check_call(ix, filters, n_filters, query_subset, B, true));
  else
    NP_TRY(check_subsets(subset_ids, subset_offsets, n_subsets, query_subset, query_subset, B));
  if (B > 0 && (!queries || !q_tok_offsets || !out_ids || !out_scores || !out_counts)) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B > 0 && q_tok_offsets[0] != 0) {
    set_error("Shape error: q_tok_offsets[0] must be 0");
    return NP_ERR_SHAPE;
  }
  for (int b = 0; b < B; ++b)
    if (q_tok_offsets[b + 1] < q_tok_offsets[b]) {
      set_error("Shape error: q_tok_offsets must be non-decreasing");
      return NP_ERR_SHAPE;
    }
  np_search_params sem = *params;
  sem.top_k = fetch_k;
  const int top_k = grp ? grp->pool_k : params->top_k;   // of the fused list
  const auto t0 = std::chrono::steady_clock::now();
  TextProg prog;
  if (text_exprs) prog.build_expr(ix, text_exprs, B); else prog.build(ix, text_queries, B);
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  if (B == 0)   // (the semantic call's own checks)
    return search_batch_in_use(ix, use, nullptr, nullptr, nullptr, 0, dim, &sem, CallSubsets(), nullptr, nullptr, nullptr);
  HostScope scope;
  NP_TRY(scope.resolve(ix, use, subset_ids, subset_offsets, n_subsets, query_subset, filters, B));
  const int64_t ntok = q_tok_offsets[B];
  const size_t b_q = up256((size_t)std::max<int64_t>(ntok, 1) * dim * 4), b_qoff = up256((size_t)(B + 1) * 4);
  ResultStage sem_l(B, fetch_k), kw_l(B, fetch_k), res(B, top_k);   // the two lists stay on the device
  GroupStage grouped(B, grp ? params->top_k : 0, grp ? grp->group_size : 0);   // (and the fused one, where it is collapsed)
  const size_t head = grp ? grouped.bytes() : res.bytes();   // what comes back through the pinned area
  const size_t user = b_q + b_qoff + scope.stage_bytes() + sem_l.bytes() + kw_l.bytes() + res.bytes() + (grp ? grouped.bytes() : 0);
  TextPlan plan;
  NP_TRY(text_plan_for(ix, (int64_t)user + scope.budget_extra(), prog, B, fetch_k, scope.any, &plan));
  NP_TRY(use.arena().reserve(user + text_arena_bytes(ix, plan, prog, fetch_k, scope.any)));
  void* pin = nullptr;   // the results, the keyword programs behind them
  NP_TRY(use.pin(head + prog.bytes, &pin));
  Carver carve{use.arena().as<char>()};
  float* d_q = (float*)carve.take(b_q);
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  CallSubsets sub;
  NP_TRY(scope.place(carve, st, &sub));
  sem_l.carve(carve);
  kw_l.carve(carve);
  res.carve(carve);
  if (grp) grouped.carve(carve);
  if (ntok > 0) NP_HIP(hipMemcpyAsync(d_q, queries, (size_t)ntok * dim * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  NP_TRY(search_batch_in_use(ix, use, d_q, d_qoff, q_tok_offsets, B, dim, &sem, sub, sem_l.d_ids, sem_l.d_sc, sem_l.d_cnt));
  int64_t visited = 0;
  NP_TRY(text_run(ix, use, carve.at, (char*)pin + head, plan, prog, fetch_k, sub, kw_l.d_ids, kw_l.d_sc, kw_l.d_cnt,
                  stats ? &visited : nullptr, nullptr, nullptr));
  NP_TRY(fuse_launch(st, fusion, alpha, top_k, B, sem_l.d_ids, sem_l.d_sc, sem_l.d_cnt, fetch_k, kw_l.d_ids, kw_l.d_sc, kw_l.d_cnt, fetch_k,
                     res.d_ids, res.d_sc, res.d_cnt));
  if (grp) {
    NP_TRY(collapse_launch(ix, st, params->top_k, grp->group_size, B, res.d_ids, res.d_sc, res.d_cnt, top_k, grouped.d_ids,
                           grouped.d_sc, grouped.d_group, grouped.d_members, grouped.d_total, grouped.d_cnt));
    NP_TRY(grouped.fetch(pin, st, true));
  } else {
    NP_TRY(res.fetch(pin, st));
  }
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  if (grp)
    grouped.deliver(out_ids, out_scores, grp->out_group, grp->out_members, grp->out_total, out_counts);
  else
    res.deliver(out_ids, out_scores, out_counts);
  if (stats) {
    stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->n_queries = B;
    stats->n_ivf_ids = visited;
  }
  return NP_OK;
}

int np_hip_search_hybrid(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                         const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k, float alpha,
                         int32_t fusion, const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                         const int32_t* query_subset, const np_filter* filters, int32_t n_filters, int64_t* out_ids,
                         float* out_scores, int32_t* out_counts, np_stats* stats) {
  return hybrid_host(ix, queries, q_tok_offsets, B, dim, params, text_queries, fetch_k, alpha, fusion, subset_ids, subset_offsets,
                     n_subsets, query_subset, filters, n_filters, out_ids, out_scores, out_counts, stats, nullptr);
}

int np_hip_search_hybrid_expr(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                              const np_search_params* params, const np_text_expr* text_queries, int32_t fetch_k, float alpha,
                              int32_t fusion, const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                              const int32_t* query_subset, const np_filter* filters, int32_t n_filters, int64_t* out_ids,
                              float* out_scores, int32_t* out_counts, np_stats* stats) {
  return hybrid_host(ix, queries, q_tok_offsets, B, dim, params, nullptr, fetch_k, alpha, fusion, subset_ids, subset_offsets,
                     n_subsets, query_subset, filters, n_filters, out_ids, out_scores, out_counts, stats, nullptr, text_queries);
}

int np_hip_search_hybrid_grouped(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                 const np_search_params* params, const np_text_query* text_queries, int32_t fetch_k, float alpha,
                                 int32_t fusion, const int64_t* subset_ids, const int64_t* subset_offsets, int64_t n_subsets,
                                 const int32_t* query_subset, const np_filter* filters, int32_t n_filters, int32_t pool_k,
                                 int32_t group_size, int64_t* out_ids, float* out_scores, int32_t* out_group,
                                 int32_t* out_members, int32_t* out_total, int32_t* out_counts, np_stats* stats) {
  const GroupCall grp{pool_k, group_size, out_group, out_members, out_total};
  return hybrid_host(ix, queries, q_tok_offsets, B, dim, params, text_queries, fetch_k, alpha, fusion, subset_ids, subset_offsets,
                     n_subsets, query_subset, filters, n_filters, out_ids, out_scores, out_counts, stats, &grp);
}

// the three sharded entries and their _expr forms (exprs != NULL: tree queries in place of `queries`; a NULL batch gets the flat
// form's checks, as in text_host)
static int text_sharded(const np_index* ix, np_comm* c, const np_text_query* queries, const np_text_expr* exprs, int32_t B, int32_t top_k,
                        const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                        int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                        int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(text_check_sharded_args(ix, c, queries, exprs, B, top_k, d_out_ids, d_out_scores, d_out_counts, stream));
  NP_TRY(check_device_subsets(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, B));
  if (B == 0) return NP_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  return text_sharded_locked(ix, c, queries, exprs, B, top_k,
                             CallSubsets::device(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset), NP_OK,
                             nullptr, d_out_ids, d_out_scores, d_out_counts, (hipStream_t)stream);
}

static int text_sharded_filtered(const np_index* ix, np_comm* c, const np_text_query* queries, const np_text_expr* exprs, int32_t B,
                                 int32_t top_k, const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                 int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(text_check_sharded_args(ix, c, queries, exprs, B, top_k, d_out_ids, d_out_scores, d_out_counts, stream));
  NP_TRY(check_sharded_filters("Filter failed", filters, n_filters, query_filter, B));
  if (B == 0) return NP_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(ix->device);
  ShardFilterScope scope;   // (nHit never looks at the scope: the keyword pass needs no global lengths)
  scope.eval(ix, c, (hipStream_t)stream, filters, n_filters, query_filter, B);
  return text_sharded_locked(ix, c, queries, exprs, B, top_k, scope.call(), scope.rc0, scope.msg0.c_str(), d_out_ids, d_out_scores,
                             d_out_counts, (hipStream_t)stream);
}

int np_hip_text_search_sharded(const np_index* ix, np_comm* c, const np_text_query* queries, int32_t B, int32_t top_k,
                               const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                               int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                               int32_t* d_out_counts, void* stream) {
  return text_sharded(ix, c, queries, nullptr, B, top_k, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset,
                      d_out_ids, d_out_scores, d_out_counts, stream);
}

int np_hip_text_search_sharded_expr(const np_index* ix, np_comm* c, const np_text_expr* queries, int32_t B, int32_t top_k,
                                    const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                    int64_t n_subsets, const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                                    int32_t* d_out_counts, void* stream) {
  return text_sharded(ix, c, nullptr, queries, B, top_k, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets,
                      d_query_subset, d_out_ids, d_out_scores, d_out_counts, stream);
}

int np_hip_text_search_sharded_filtered(const np_index* ix, np_comm* c, const np_text_query* queries, int32_t B, int32_t top_k,
                                        const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                        int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream) {
  return text_sharded_filtered(ix, c, queries, nullptr, B, top_k, filters, n_filters, query_filter, d_out_ids, d_out_scores,
                               d_out_counts, stream);
}

int np_hip_text_search_sharded_expr_filtered(const np_index* ix, np_comm* c, const np_text_expr* queries, int32_t B, int32_t top_k,
                                             const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                             int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts, void* stream) {
  return text_sharded_filtered(ix, c, nullptr, queries, B, top_k, filters, n_filters, query_filter, d_out_ids,
                               d_out_scores, d_out_counts, stream);
}

static int hybrid_sharded(const np_index* ix, np_comm* c, const float* d_queries, const int32_t* d_q_tok_offsets,
                          const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                          const np_text_query* text_queries, const np_text_expr* text_exprs, int32_t fetch_k, float alpha,
                          int32_t fusion, const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                          const int64_t* h_subset_offsets, int64_t n_subsets, const int32_t* d_query_subset, const np_filter* filters,
                          int32_t n_filters, const int32_t* query_filter, int64_t* d_out_ids, float* d_out_scores,
                          int32_t* d_out_counts, void* stream) {
  clear_error();
  if (!params) {
    set_error("Search failed: NULL index or params");
    return NP_ERR_INVALID_ARGUMENT;
  }
  // arguments every rank sees alike: before the lock and the first collective
  NP_TRY(text_check_sharded_args(ix, c, text_queries, text_exprs, B, fetch_k, d_out_ids, d_out_scores, d_out_counts, stream));
  NP_TRY(fuse_check(fusion, alpha, params->top_k, B, fetch_k, fetch_k));
  if (filters)
    NP_TRY(check_sharded_filters("Filter failed", filters, n_filters, query_filter, B));
  else
    NP_TRY(check_device_subsets(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, B));
  if (B > 0 && (!d_queries || !d_q_tok_offsets || !h_q_tok_offsets)) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B == 0) return NP_OK;
  np_search_params sem = *params;
  sem.top_k = fetch_k;
  const int top_k = params->top_k;
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(ix->device);
  // the two global lists, [B][fetch_k] each, stay in the communicator
  ResultStage sem_l(B, fetch_k), kw_l(B, fetch_k);
  NP_TRY(c->lists.reserve(sem_l.bytes() + kw_l.bytes()));
  Carver carve{c->lists.as<char>()};
  sem_l.carve(carve);
  kw_l.carve(carve);
  // the scope: the caller's CSR, or the filters over this shard's columns with their local lengths for the probe scaling
  ShardFilterScope scope;
  if (filters) scope.eval(ix, c, st, filters, n_filters, query_filter, B);
  const CallSubsets sub =
      filters ? scope.call() : CallSubsets::device(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset);
  const ShardSubsets ss = filters ? scope.shard() : ShardSubsets::csr(sub);
  // With the host-side check a failed semantic pass has ended on every rank at the same exchange (each read the same status
  // words): all leave.  Otherwise the failing rank has returned its own error after taking part in every exchange, while its peers
  // carry on with an abandoned list: it still owes them the exchanges of the keyword pass, with empty data and its status.
  const int rc_sem = search_batch_sharded_locked(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, &sem, ss, sem_l.d_ids,
                                                 sem_l.d_sc, sem_l.d_cnt, stream, scope.rc0, scope.msg0.c_str());
  const std::string msg_sem = rc_sem != NP_OK ? np_hip_last_error() : "";
  if (rc_sem != NP_OK && c->host_check()) return rc_sem;
  const int rc_kw = text_sharded_locked(ix, c, text_queries, text_exprs, B, fetch_k, sub, rc_sem, msg_sem.c_str(), kw_l.d_ids, kw_l.d_sc, kw_l.d_cnt, st);
  if (rc_kw != NP_OK) return rc_kw;
  // every rank holds both global lists: every rank fuses.  (An abandoned list carries count -1: the fusion clamps it to an empty
  // list, and the count that leaves is the abandoned one.)
  NP_TRY(fuse_launch(st, fusion, alpha, top_k, B, sem_l.d_ids, sem_l.d_sc, sem_l.d_cnt, fetch_k, kw_l.d_ids, kw_l.d_sc, kw_l.d_cnt, fetch_k,
                     d_out_ids, d_out_scores, d_out_counts));
  hybrid_abandon_kernel<<<(unsigned)((B + 255) / 256), 256, 0, st>>>(sem_l.d_cnt, kw_l.d_cnt, B, d_out_counts);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int np_hip_search_hybrid_sharded(const np_index* ix, np_comm* c, const float* d_queries, const int32_t* d_q_tok_offsets,
                                 const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                                 const np_text_query* text_queries, int32_t fetch_k, float alpha, int32_t fusion,
                                 const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                 int64_t n_subsets, const int32_t* d_query_subset, const np_filter* filters, int32_t n_filters,
                                 const int32_t* query_filter, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                 void* stream) {
  return hybrid_sharded(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, text_queries, nullptr, fetch_k, alpha,
                        fusion, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, filters, n_filters,
                        query_filter, d_out_ids, d_out_scores, d_out_counts, stream);
}

int np_hip_search_hybrid_sharded_expr(const np_index* ix, np_comm* c, const float* d_queries, const int32_t* d_q_tok_offsets,
                                      const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                                      const np_text_expr* text_queries, int32_t fetch_k, float alpha, int32_t fusion,
                                      const int64_t* d_subset_ids, const int64_t* d_subset_offsets, const int64_t* h_subset_offsets,
                                      int64_t n_subsets, const int32_t* d_query_subset, const np_filter* filters, int32_t n_filters,
                                      const int32_t* query_filter, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                      void* stream) {
  return hybrid_sharded(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, nullptr, text_queries,
                        fetch_k, alpha, fusion, d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, filters,
                        n_filters, query_filter, d_out_ids, d_out_scores, d_out_counts, stream);
}

}  // extern "C"
