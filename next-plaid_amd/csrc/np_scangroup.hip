// np_scangroup.hip -- np_hip_search_exact_grouped: the true top_k GROUPS of every query over every document of its scope, each
// with its best group_size documents: np_hip_collapse of the complete np_hip_search_exact list, without that list.
//
// Built on np_scan.hip's stages, which this file includes: the two are one translation unit, np_scan.hip's text is as it was.
// A scan pass leaves keys[query][document] = okey(score) << 32 | ~id (0 = out of scope); instead of selecting documents,
//   group_fold_kernel    reduces a pass into best[query][group] (64-bit maximum: higher score, then lower id) and
//                        count[query][group] (in-scope documents).  Consecutive documents usually share a group (units of a
//                        file), so a wave first reduces its 64 documents by runs of equal groups with shuffles and issues one
//                        atomicMax and one atomicAdd per run.  Maximum and sum commute: arrival order decides nothing.
//   scan_topk_kernel     np_scan.hip's, over the row best[query][0 .. n_groups): the top_k leaders in rank order.
//   group_rows_kernel    group, total, members, the leader and the padding of every output row; for group_size > 1 it turns the
//                        count row into "ordinal + 1 of a selected group, 0 otherwise".
//   group_scope_kernel   the document bitmap of every query's selected groups inside its scope: the subsets of a second scan,
//                        which re-scores those documents alone (the same kernel, hence the same bits).
//   group_member_kernel  a key of that scan enters its group's group_size slots by a cascade of atomicMax: slot j keeps the
//                        larger of what it holds and what arrives and passes the smaller on.  Slot j ends as the (j+1)-th
//                        largest key of the group whatever the arrival order (a slot ends as the maximum of the multiset it
//                        was offered and offers everything else on: induction over j).
//   group_emit_kernel    keys of the slots to ids and score bits.
#include "np_scan.hip"
#include "np_group_plan.h"

#include <chrono>

namespace np {

typedef unsigned long long u64;

__global__ void __launch_bounds__(256) group_fold_kernel(const uint64_t* __restrict__ keys, int64_t P, int n, int64_t d0,
                                                         const int32_t* __restrict__ doc_group, int64_t NG, u64* best,
                                                         int32_t* count) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int64_t dl = (int64_t)blockIdx.x * 256 + threadIdx.x;
  u64 key = dl < n ? keys[(int64_t)b * P + dl] : 0ull;
  const int g = key ? doc_group[d0 + dl] : -1;   // a document out of scope ends a run
  int c = key ? 1 : 0;
  // segmented inclusive scan over the wave: `start` = the first lane of this lane's run of equal groups
  const int gp = __shfl_up(g, 1);
  int start = (lane == 0 || gp != g) ? lane : 0;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(start, d);
    if (lane >= d) start = max(start, o);
  }
  for (int d = 1; d < 64; d <<= 1) {
    const u64 ok = __shfl_up(key, d);
    const int oc = __shfl_up(c, d);
    if (lane - d >= start) {
      key = ok > key ? ok : key;
      c += oc;
    }
  }
  const int gn = __shfl_down(g, 1);
  if (g >= 0 && (lane == 63 || gn != g)) {   // the run's last lane holds its maximum and its length
    atomicMax(&best[(int64_t)b * NG + g], key);
    atomicAdd(&count[(int64_t)b * NG + g], c);
  }
}

// a non-finite score comes back as NaN, as scan_topk_kernel returns it
__device__ __forceinline__ uint32_t key_score_bits(u64 key) {
  const uint32_t ks = (uint32_t)(key >> 32);
  return ks ? __float_as_uint(unkey(ks)) : 0x7FC00000u;
}
__device__ __forceinline__ int64_t key_doc(u64 key) { return (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }

struct GroupRowsP {
  const u64* lead;            // [S][top_k] the leaders' keys in rank order, 0-padded (scan_topk_kernel's best)
  const int32_t* n_lead;      // [S]
  int32_t* count;             // [S][NG]
  int64_t NG;
  const int32_t* doc_group;
  int top_k, group_size;
  u64* slots;                 // [S][top_k][group_size] or NULL (group_size == 1)
  int64_t* out_ids;           // [S][top_k][group_size]
  uint32_t* out_scores;
  int32_t *out_group, *out_members, *out_total;   // [S][top_k]
};

// one workgroup per query: np_hip_collapse's row -- padding included -- with every group's leader in slot 0
__global__ void __launch_bounds__(1024) group_rows_kernel(GroupRowsP p) {
  const int b = blockIdx.x, tid = threadIdx.x, nsel = p.n_lead[b], gs = p.group_size;
  int32_t* cp = p.count + (int64_t)b * p.NG;
  for (int i = tid; i < p.top_k * gs; i += 1024) {
    const int j = i / gs;
    const u64 key = (i == j * gs && j < nsel) ? p.lead[(int64_t)b * p.top_k + j] : 0ull;
    const int64_t o = (int64_t)b * p.top_k * gs + i;
    p.out_ids[o] = key ? key_doc(key) : 0;
    p.out_scores[o] = key ? key_score_bits(key) : 0u;
    if (p.slots) p.slots[o] = 0ull;
    if (i == j * gs) {
      const int grp = key ? p.doc_group[key_doc(key)] : 0, total = key ? cp[grp] : 0;
      const int64_t r = (int64_t)b * p.top_k + j;
      p.out_group[r] = grp;
      p.out_total[r] = total;
      p.out_members[r] = min(total, gs);
    }
  }
  if (!p.slots) return;
  __syncthreads();   // every total is read: the count row becomes "ordinal + 1 of a selected group"
  for (int64_t i = tid; i < p.NG; i += 1024) cp[i] = 0;
  __syncthreads();
  for (int j = tid; j < nsel; j += 1024) cp[p.doc_group[key_doc(p.lead[(int64_t)b * p.top_k + j])]] = j + 1;
}

// mbits[b][w]: the documents of word w that are in query b's scope and in one of its selected groups; mrow[b] = b
__global__ void __launch_bounds__(256) group_scope_kernel(const int32_t* __restrict__ qrow, const uint32_t* __restrict__ docbits,
                                                          int64_t NW, int64_t n_docs, const int32_t* __restrict__ doc_group,
                                                          const int32_t* __restrict__ count, int64_t NG, uint32_t* mbits,
                                                          int32_t* mrow) {
  const int b = blockIdx.y;
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w == 0) mrow[b] = b;
  if (w >= NW) return;
  const int row = qrow ? qrow[b] : -1;
  const uint32_t in = row < 0 ? 0xFFFFFFFFu : docbits[(int64_t)row * NW + w];
  uint32_t out = 0;
  for (int i = 0; i < 32 && w * 32 + i < n_docs; ++i)
    if (((in >> i) & 1u) && count[(int64_t)b * NG + doc_group[w * 32 + i]] != 0) out |= 1u << i;
  mbits[(int64_t)b * NW + w] = out;
}

// Non-zero keys of one group are distinct (distinct documents).  The last slot only grows, so a key below what it holds now
// can never end in a slot.
__global__ void __launch_bounds__(256) group_member_kernel(const uint64_t* __restrict__ keys, int64_t P, int n, int64_t d0,
                                                           const int32_t* __restrict__ doc_group, const int32_t* __restrict__ count,
                                                           int64_t NG, int top_k, int group_size, u64* slots) {
  const int b = blockIdx.y;
  const int64_t dl = (int64_t)blockIdx.x * 256 + threadIdx.x;
  u64 key = dl < n ? keys[(int64_t)b * P + dl] : 0ull;
  if (!key) return;
  const int ord = count[(int64_t)b * NG + doc_group[d0 + dl]] - 1;
  if (ord < 0) return;
  u64* slot = slots + ((int64_t)b * top_k + ord) * group_size;
  if (key <= __hip_atomic_load(&slot[group_size - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
  for (int j = 0; j < group_size && key; ++j) {
    const u64 old = atomicMax(&slot[j], key);
    if (old < key) key = old;   // the slot took the key: what it held moves on
  }
}

// an empty slot keeps the padding group_rows_kernel wrote
__global__ void __launch_bounds__(256) group_emit_kernel(const u64* __restrict__ slots, int64_t n, int64_t* __restrict__ out_ids,
                                                         uint32_t* __restrict__ out_scores) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const u64 key = i < n ? slots[i] : 0ull;
  if (!key) return;
  out_ids[i] = key_doc(key);
  out_scores[i] = key_score_bits(key);
}

// ---- host ------------------------------------------------------------------------------------------------------------
// bytes of the arena per query of a slice beyond the scan's own: the table rows (12 bytes per group), the leaders' scratch
// rows, the member slots and the member scan's bitmap
static int64_t group_per_query(const DeviceIndex* ix, int top_k, int group_size) {
  const int64_t NW = std::max<int64_t>((ix->n_docs + 31) / 32, 1);
  return (int64_t)up256((size_t)ix->n_groups * 8) + (int64_t)up256((size_t)ix->n_groups * 4) + (int64_t)up256((size_t)top_k * 12) +
         (int64_t)up256((size_t)top_k * group_size * 8) + (int64_t)up256((size_t)NW * 4) + 4;
}

// one scan of the slice's queries over every document, pass by pass; after a pass `fold` or the member kernel takes its keys
static int group_scan_passes(const DeviceIndex* ix, hipStream_t st, ScanP sp, int groups, bool bf16, int Sn, int top_k,
                             int group_size, u64* best, int32_t* count, u64* slots) {
  const int64_t NG = ix->n_groups;
  for (int64_t d0 = 0; d0 < ix->n_docs; d0 += sp.P) {
    const int n = (int)std::min<int64_t>(sp.P, ix->n_docs - d0);
    sp.d0 = d0;
    sp.n = n;
    const int64_t nblk = ((int64_t)n + 4 * NP_SCAN_DPW - 1) / (4 * NP_SCAN_DPW);
    const unsigned gx = (unsigned)std::min<int64_t>(nblk, std::max(1, 2048 / groups));
    int rc;
    switch (ix->dim) {
      case 32: rc = launch_scan_dim<32>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
      case 64: rc = launch_scan_dim<64>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
      case 96: rc = launch_scan_dim<96>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
      default: rc = launch_scan_dim<128>(st, sp, gx, (unsigned)groups, ix->nbits, bf16); break;
    }
    NP_TRY(rc);
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)Sn);
    if (best)
      group_fold_kernel<<<grid, 256, 0, st>>>(sp.keys, sp.P, n, d0, ix->d_groups.get(), NG, best, count);
    else
      group_member_kernel<<<grid, 256, 0, st>>>(sp.keys, sp.P, n, d0, ix->d_groups.get(), count, NG, top_k, group_size, slots);
    NP_HIP(hipGetLastError());
  }
  return NP_OK;
}

// The whole batch on device buffers: slices of S queries, passes of P documents (scan_plan).  `base`: the part of the arena this
// function may carve.  Nothing waits.
static int group_scan_run(const DeviceIndex* ix, hipStream_t st, char* base, const ScanPlan& plan, const float* d_q,
                          const int32_t* d_qoff, const int32_t* h_qoff, int B, int top_k, int group_size, int precision,
                          const CallSubsets& sub, const GroupStage& out) {
  const int S = plan.S;
  const int64_t NW = std::max<int64_t>((ix->n_docs + 31) / 32, 1), NG = ix->n_groups, nslot = (int64_t)top_k * group_size;
  const bool bf16 = precision == 3 && ix->nbits != 8;
  const bool subsets = sub.n > 0;
  Carver carve{base};
  int32_t* tile_info = (int32_t*)carve.take((size_t)S * NP_SCAN_MAX_TILES * 4);
  int32_t* qrow = (int32_t*)carve.take((size_t)S * 4);
  int32_t* mrow = (int32_t*)carve.take((size_t)S * 4);
  char* Q = carve.take((size_t)S * up256((size_t)ix->dim * NP_SCAN_MAX_QUERY_TOKENS * 4));
  u64* lead = (u64*)carve.take((size_t)S * up256((size_t)top_k * 8));
  uint32_t* docbits = subsets ? (uint32_t*)carve.take((size_t)S * up256((size_t)NW * 4)) : nullptr;
  uint64_t* keys = (uint64_t*)carve.take((size_t)S * plan.P * 8);
  u64* best = (u64*)carve.take((size_t)S * NG * 8);
  int32_t* count = (int32_t*)carve.take((size_t)S * NG * 4);
  int64_t* lead_ids = (int64_t*)carve.take((size_t)S * top_k * 8);   // scan_topk_kernel's outputs: only its counts are used
  float* lead_sc = (float*)carve.take((size_t)S * top_k * 4);
  u64* slots = group_size > 1 ? (u64*)carve.take((size_t)S * nslot * 8) : nullptr;
  uint32_t* mbits = group_size > 1 ? (uint32_t*)carve.take((size_t)S * NW * 4) : nullptr;
  int nselp = 1;
  while (nselp < top_k) nselp <<= 1;
  const size_t topk_lds = (size_t)nselp * 8;
  if (topk_lds > 48 * 1024)
    NP_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&scan_topk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)topk_lds));
  for (int s0 = 0; s0 < B; s0 += S) {
    const int Sn = std::min(S, B - s0);
    int max_tiles = 1;
    const int groups = scan_pack_groups(h_qoff + s0, Sn, ix->tune.scan_tiles, nullptr, &max_tiles);
    scan_groups_kernel<<<1, 64, 0, st>>>(d_qoff + s0, Sn, ix->tune.scan_tiles, tile_info);
    scan_prep_kernel<<<groups, 256, 0, st>>>(d_q, d_qoff + s0, ix->ldim, ix->dim, 32 * max_tiles, tile_info,
                                            bf16 ? nullptr : (float*)Q, bf16 ? (__bf16*)Q : nullptr);
    if (subsets)   // (every id of the call: a slice's own range is the scan's refinement)
      NP_TRY(subset_doc_rows(ix, st, sub.d_ids, sub.d_off, sub.d_qsub + s0, sub.n, sub.total, 0, sub.total, Sn, NW, docbits, qrow));
    NP_HIP(hipMemsetAsync(best, 0, (size_t)Sn * NG * 8, st));
    NP_HIP(hipMemsetAsync(count, 0, (size_t)Sn * NG * 4, st));
    ScanP sp;
    sp.Qf = bf16 ? nullptr : (const float*)Q;
    sp.Qb = bf16 ? (const __bf16*)Q : nullptr;
    sp.tile_info = tile_info;
    sp.qoff = d_qoff + s0;
    sp.TW = 32 * max_tiles;
    sp.centroids = ix->d_centroids.get();
    sp.wlut = ix->d_wlut.get();
    sp.codes = ix->codes();
    sp.residuals = ix->d_residuals.get();
    sp.doc_off = ix->d_doc_offsets.get();
    sp.pad_ss = ix->pad_ss;
    sp.doc_begin = ix->doc_begin;
    sp.P = plan.P;
    sp.qrow = subsets ? qrow : nullptr;
    sp.docbits = docbits;
    sp.NW = NW;
    sp.keys = keys;
    sp.ctr = nullptr;
    NP_TRY(group_scan_passes(ix, st, sp, groups, bf16, Sn, top_k, group_size, best, count, nullptr));
    ScanTopkP tp;
    tp.keys = (const uint64_t*)best;
    tp.P = NG;
    tp.n = (int)NG;
    tp.n_prev = 0;
    tp.best = (uint64_t*)lead;
    tp.top_k = top_k;
    tp.NSELP = nselp;
    tp.out_ids = lead_ids;
    tp.out_scores = lead_sc;
    tp.out_counts = out.d_cnt + s0;
    scan_topk_kernel<<<Sn, 1024, topk_lds, st>>>(tp);
    GroupRowsP rp{lead, out.d_cnt + s0, count, NG, ix->d_groups.get(), top_k, group_size, slots, out.d_ids + s0 * nslot,
                  (uint32_t*)out.d_sc + s0 * nslot, out.d_group + (int64_t)s0 * top_k, out.d_members + (int64_t)s0 * top_k,
                  out.d_total + (int64_t)s0 * top_k};
    group_rows_kernel<<<Sn, 1024, 0, st>>>(rp);
    NP_HIP(hipGetLastError());
    if (group_size > 1) {
      group_scope_kernel<<<dim3((unsigned)((NW + 255) / 256), (unsigned)Sn), 256, 0, st>>>(sp.qrow, docbits, NW, ix->n_docs,
                                                                                           ix->d_groups.get(), count, NG, mbits, mrow);
      sp.qrow = mrow;
      sp.docbits = mbits;
      NP_TRY(group_scan_passes(ix, st, sp, groups, bf16, Sn, top_k, group_size, nullptr, count, slots));
      const int64_t n = (int64_t)Sn * nslot;
      group_emit_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(slots, n, rp.out_ids, rp.out_scores);
      NP_HIP(hipGetLastError());
    }
  }
  return NP_OK;
}

// np_hip_search_exact_grouped and its filtered form: np_hip_search_exact's checks, scope and staging (scan_host) with the
// grouped entries' six output regions
static int group_scan_host(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                           int32_t top_k, int32_t group_size, int32_t precision, const int64_t* subset_ids,
                           const int64_t* subset_offsets, int64_t n_subsets, const int32_t* query_subset, const np_filter* filters,
                           int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members, int32_t* out_total,
                           int32_t* out_counts, np_stats* stats) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  if (stats) memset(stats, 0, sizeof *stats);
  const char* why = ix ? "" : "NULL index";
  if (ix && ix->opts.shard_count > 1)
    why = "a sharded handle is refused: a group's members can lie on several shards, so per-shard grouped lists do not merge exactly";
  if (*why || group_check_args(ix->n_groups > 0, top_k, group_size, B, 1, &why) != 0) {   // (stride 1: the entry takes none)
    set_error("Search failed: %s (top_k=%d group_size=%d)", why, top_k, group_size);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B > 0 && !q_tok_offsets) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(scan_validate(ix, B, dim, top_k, precision, B > 0 ? q_tok_offsets : nullptr));
  if (filters)
    NP_TRY(filter_check_call(ix, filters, (int32_t)n_subsets, query_subset, B, true));
  else
    NP_TRY(check_subsets(subset_ids, subset_offsets, n_subsets, query_subset, query_subset, B));
  if (B == 0) return NP_OK;
  if (!queries || !out_ids || !out_scores || !out_group || !out_members || !out_total || !out_counts) {
    set_error("Search failed: NULL buffer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const auto t0 = std::chrono::steady_clock::now();
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  hipStream_t st = use.stream;
  HostScope scope;
  NP_TRY(scope.resolve(ix, use, subset_ids, subset_offsets, n_subsets, query_subset, filters, B));
  const int64_t ntok = q_tok_offsets[B];
  const size_t b_q = up256((size_t)std::max<int64_t>(ntok, 1) * dim * 4), b_qoff = up256((size_t)(B + 1) * 4);
  GroupStage res(B, top_k, group_size);
  const size_t user = b_q + b_qoff + scope.stage_bytes() + res.bytes();
  // the scan's plan -- S queries a slice, P documents a pass -- with the tables' bytes added to a query's share
  const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
  const int64_t per_query = scan_per_query(ix, top_k, scope.any) + group_per_query(ix, top_k, group_size);
  ScanPlan plan;
  if (!scan_plan(budget, (int64_t)user + scope.budget_extra() + 8192, per_query, ix->n_docs, B, ix->opts.max_batch, ix->tune.scan_docs,
                 &plan)) {
    set_error("Search failed: one query's table over %lld groups does not fit the workspace budget of %lld bytes",
              (long long)ix->n_groups, (long long)budget);
    return NP_ERR_OUT_OF_MEMORY;
  }
  NP_TRY(use.arena().reserve(user + 8192 + (size_t)plan.S * (size_t)per_query + up256((size_t)plan.S * plan.P * 8)));
  void* pin = nullptr;
  NP_TRY(use.pin(res.bytes(), &pin));
  Carver carve{use.arena().as<char>()};
  float* d_q = (float*)carve.take(b_q);
  int32_t* d_qoff = (int32_t*)carve.take(b_qoff);
  CallSubsets sub;
  NP_TRY(scope.place(carve, st, &sub));
  res.carve(carve);
  if (ntok > 0) NP_HIP(hipMemcpyAsync(d_q, queries, (size_t)ntok * dim * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipMemcpyAsync(d_qoff, q_tok_offsets, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, st));
  NP_TRY(group_scan_run(ix, st, carve.at, plan, d_q, d_qoff, q_tok_offsets, B, top_k, group_size, precision, sub, res));
  NP_TRY(res.fetch(pin, st, true));
  NP_TRY(use.end());
  NP_HIP(hipStreamSynchronize(st));
  res.deliver(out_ids, out_scores, out_group, out_members, out_total, out_counts);
  if (stats) {
    stats->ms_total = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    stats->n_queries = B;
  }
  return NP_OK;
}

}  // namespace np

extern "C" {

int np_hip_search_exact_grouped(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B, int32_t dim,
                                int32_t top_k, int32_t group_size, int32_t precision, const int64_t* subset_ids,
                                const int64_t* subset_offsets, int64_t n_subsets, const int32_t* query_subset, int64_t* out_ids,
                                float* out_scores, int32_t* out_group, int32_t* out_members, int32_t* out_total,
                                int32_t* out_counts, np_stats* stats) {
  return group_scan_host(ix, queries, q_tok_offsets, B, dim, top_k, group_size, precision, subset_ids, subset_offsets, n_subsets,
                         query_subset, nullptr, out_ids, out_scores, out_group, out_members, out_total, out_counts, stats);
}

int np_hip_search_exact_grouped_filtered(const np_index* ix, const float* queries, const int32_t* q_tok_offsets, int32_t B,
                                         int32_t dim, int32_t top_k, int32_t group_size, int32_t precision,
                                         const np_filter* filters, int32_t n_filters, const int32_t* query_filter,
                                         int64_t* out_ids, float* out_scores, int32_t* out_group, int32_t* out_members,
                                         int32_t* out_total, int32_t* out_counts, np_stats* stats) {
  static const np_filter none{};   // n_filters == 0: nothing to check or evaluate, but still the filtered call's checks
  return group_scan_host(ix, queries, q_tok_offsets, B, dim, top_k, group_size, precision, nullptr, nullptr, n_filters,
                         query_filter, filters ? filters : &none, out_ids, out_scores, out_group, out_members, out_total,
                         out_counts, stats);
}

}  // extern "C"
