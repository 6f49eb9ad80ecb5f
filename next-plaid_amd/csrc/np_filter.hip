// np_filter.hip -- metadata filters on the device: np_hip_filter_eval and the evaluation stage of the filtered searches.
//
// A filter is a postfix program over the handle's columns (include/nextplaid_hip.h).  Two kernels do the work:
//   filter_mask_kernel     one lane per document, one grid row per filter.  The program is the same for every lane of the
//                          grid, so its ops are read through uniform (scalar) loads and the stack pointer is uniform too: a
//                          lane's stack is two 32-bit registers, "true" bits and "known" bits, bit d = the entry at depth d.
//                          Column reads are coalesced SoA reads, IN is a binary search of the sorted constants, and a wave's
//                          64 results leave as one ballot word (bits past the last document are zero).
//   filter_compact_kernel  ordered compaction: per-word popcounts (filter_count_kernel), an exclusive scan across blocks
//                          (filter_scan_kernel), then every wave writes the ids of its words in ascending order, one
//                          coalesced store per 64-document word.  No atomic decides the position of an id.
// A table of per-(filter, document chunk) totals, scanned once more on the device, is at the same time the CSR's offsets and
// the place of every chunk's segment in it; the host reads that table back and nothing else.
#include "np_internal.h"
#include "np_filter_plan.h"
#include <chrono>
#include <string.h>

namespace np {

constexpr int FILTER_TPB = 256;   // lanes of a mask block = words of a compaction block

struct FilterEvalP {
  const FilterCol* cols;
  const np_filter_op* ops;      // all filters' ops; first_value already points into `values`
  const int32_t* op_begin;      // [n_filters + 1]
  const int64_t* values;
  int32_t f0;                   // first filter of the chunk
  int64_t d0, n;                // the chunk's documents [d0, d0 + n) of the shard
  int64_t nw;                   // mask words per filter of the chunk (blocks * 256)
  unsigned long long* mask;     // [chunk filters][nw]
  const uint32_t* match_bits;   // NP_F_MATCH: the bitmaps over codes of the call's match passes (first_value = a bitmap's word)
};

template <class T>
__device__ __forceinline__ bool filter_cmp(int arg, T x, T v) {
  switch (arg) {
    case 0: return x == v;
    case 1: return x != v;
    case 2: return x < v;
    case 3: return x <= v;
    case 4: return x > v;
    default: return x >= v;
  }
}

template <class T, class Load>
__device__ __forceinline__ bool filter_in(T x, const int64_t* __restrict__ v, int n, Load as) {
  int lo = 0, hi = n;   // first entry >= x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (as(v[mid]) < x) lo = mid + 1; else hi = mid;
  }
  return lo < n && as(v[lo]) == x;
}

__global__ void __launch_bounds__(FILTER_TPB) filter_mask_kernel(FilterEvalP p) {
  const int f = p.f0 + (int)blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * FILTER_TPB + threadIdx.x;   // document of the chunk
  const bool live = i < p.n;
  const int64_t d = p.d0 + (live ? i : p.n - 1);                      // idle lanes read the last document
  const int ob = p.op_begin[f], oe = p.op_begin[f + 1];
  uint32_t T = 0, K = 0;   // bit s: stack entry s is TRUE / is known (T is a subset of K)
  int sp = 0;              // uniform
  for (int o = ob; o < oe; ++o) {
    const np_filter_op op = p.ops[o];   // uniform address
    if (op.op <= NP_F_IS_NULL || op.op == NP_F_MATCH) {
      const FilterCol c = p.cols[op.column];
      const bool valid = c.valid ? ((c.valid[d >> 5] >> (d & 31)) & 1u) != 0 : true;
      bool t = false, k = valid;
      if (op.op == NP_F_IS_NULL) {
        t = !valid;
        k = true;
      } else if (op.op == NP_F_MATCH) {
        // every code of the handle's rows is below the text's n_strings (np_hip_index_set_column_text), NULL rows included
        const uint32_t code = (uint32_t) static_cast<const int32_t*>(c.data)[d];
        t = k && ((p.match_bits[op.first_value + (code >> 5)] >> (code & 31)) & 1u);
      } else {
        const int64_t* __restrict__ v = p.values + op.first_value;
        if (c.type == NP_COL_F64) {
          const double x = static_cast<const double*>(c.data)[d];
          if (op.op == NP_F_CMP) t = filter_cmp<double>(op.arg, x, __longlong_as_double(v[0]));
          else if (op.op == NP_F_BETWEEN) t = x >= __longlong_as_double(v[0]) && x <= __longlong_as_double(v[1]);
          else t = filter_in<double>(x, v, op.n_values, [](int64_t b) { return __longlong_as_double(b); });
        } else {
          const int64_t x = c.type == NP_COL_I64 ? static_cast<const int64_t*>(c.data)[d]
                                                 : (int64_t) static_cast<const int32_t*>(c.data)[d];
          if (op.op == NP_F_CMP) t = filter_cmp<int64_t>(op.arg, x, v[0]);
          else if (op.op == NP_F_BETWEEN) t = x >= v[0] && x <= v[1];
          else t = filter_in<int64_t>(x, v, op.n_values, [](int64_t b) { return b; });
        }
        if (op.op == NP_F_IN && (op.arg & 1) && !t) k = false;   // no match in a list that held a NULL
        t = t && k;
      }
      const uint32_t bit = 1u << sp;
      T = (T & ~bit) | (t ? bit : 0u);
      K = (K & ~bit) | (k ? bit : 0u);
      ++sp;
    } else if (op.op == NP_F_CONST) {
      const uint32_t bit = 1u << sp;
      T = (T & ~bit) | (op.arg == 1 ? bit : 0u);
      K = (K & ~bit) | (op.arg != 2 ? bit : 0u);
      ++sp;
    } else if (op.op == NP_F_NOT) {
      T ^= K & (1u << (sp - 1));   // known: flipped; unknown (T = K = 0) stays
    } else {
      const uint32_t a = sp - 2, b = sp - 1;
      const uint32_t ta = (T >> a) & 1u, tb = (T >> b) & 1u, ka = (K >> a) & 1u, kb = (K >> b) & 1u;
      const uint32_t fa = ka & ~ta, fb = kb & ~tb;
      uint32_t t, k;
      if (op.op == NP_F_AND) {
        t = ta & tb;
        k = t | ((fa | fb) & 1u);
      } else {
        t = ta | tb;
        k = t | (fa & fb & 1u);
      }
      const uint32_t bit = 1u << a;
      T = (T & ~bit) | (t << a);
      K = (K & ~bit) | (k << a);
      --sp;
    }
  }
  const unsigned long long word = __ballot(live && (T & 1u));
  if ((threadIdx.x & 63) == 0) p.mask[(int64_t)blockIdx.y * p.nw + (i >> 6)] = word;
}

// counts[filter][block] = selected documents of the block's 256 words
__global__ void __launch_bounds__(FILTER_TPB) filter_count_kernel(const unsigned long long* __restrict__ mask, int64_t nw,
                                                                  int64_t n_words, int64_t blocks,
                                                                  uint32_t* __restrict__ counts) {
  __shared__ uint32_t part[FILTER_TPB / 64];
  const int64_t w = (int64_t)blockIdx.x * FILTER_TPB + threadIdx.x;
  uint32_t c = w < n_words ? (uint32_t)__popcll(mask[(int64_t)blockIdx.y * nw + w]) : 0u;
  for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[(int64_t)blockIdx.y * blocks + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// exclusive scan of n values by one 256-lane block, in tiles: out[i] = carry + sum of in[0 .. i); returns carry + the total
// (to every lane)
template <class TIn>
__device__ int64_t filter_block_scan(const TIn* __restrict__ in, int64_t n, int64_t* __restrict__ out, int64_t carry) {
  __shared__ int64_t wsum[FILTER_TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int64_t t0 = 0; t0 < n; t0 += FILTER_TPB) {
    const int64_t i = t0 + threadIdx.x;
    const int64_t v = i < n ? (int64_t)in[i] : 0;
    int64_t inc = v;
    for (int s = 1; s < 64; s <<= 1) {
      const int64_t up = __shfl_up(inc, s);
      if (lane >= s) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t before = carry, all = carry;
    for (int w = 0; w < FILTER_TPB / 64; ++w) {
      if (w < wave) before += wsum[w];
      all += wsum[w];
    }
    if (i < n) out[i] = before + inc - v;
    carry = all;
    __syncthreads();
  }
  return carry;
}

// per filter of the chunk: base[filter][block] = selected documents in the chunk's earlier blocks; totals[...] = all of them
__global__ void __launch_bounds__(FILTER_TPB) filter_scan_kernel(const uint32_t* __restrict__ counts, int64_t blocks,
                                                                 int64_t* __restrict__ base, int64_t* __restrict__ totals,
                                                                 int64_t tot_first, int64_t tot_stride) {
  const int64_t f = blockIdx.x;
  const int64_t total = filter_block_scan(counts + f * blocks, blocks, base + f * blocks, 0);
  if (threadIdx.x == 0) totals[tot_first + f * tot_stride] = total;
}

// table[i] = sum of totals[0 .. i), table[n] = everything
__global__ void __launch_bounds__(FILTER_TPB) filter_table_kernel(const int64_t* __restrict__ totals, int64_t n,
                                                                  int64_t* __restrict__ table) {
  const int64_t total = filter_block_scan(totals, n, table, 0);
  if (threadIdx.x == 0) table[n] = total;
}

struct FilterCompactP {
  const unsigned long long* mask;
  const int64_t* base;      // [chunk filters][blocks]
  const int64_t* table;     // place of a (filter, document chunk) segment in the output; nullptr: seg_stride * filter
  int64_t table_first, table_stride;
  int64_t seg_stride;
  int64_t nw, n_words, blocks;
  int64_t first_id;         // global id of the chunk's first document
  int64_t* out;
};

__global__ void __launch_bounds__(FILTER_TPB) filter_compact_kernel(FilterCompactP p) {
  __shared__ uint32_t wsum[FILTER_TPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = blockIdx.y;
  const int64_t w = (int64_t)blockIdx.x * FILTER_TPB + threadIdx.x;
  const unsigned long long m = w < p.n_words ? p.mask[f * p.nw + w] : 0ull;
  const uint32_t c = (uint32_t)__popcll(m);
  uint32_t inc = c;
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t up = __shfl_up(inc, s);
    if (lane >= s) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  for (int x = 0; x < wave; ++x) before += wsum[x];
  const int64_t seg = p.table ? p.table[p.table_first + f * p.table_stride] : f * p.seg_stride;
  const int64_t at = seg + p.base[f * p.blocks + blockIdx.x] + before + inc - c;   // of this lane's word
  const int64_t word0 = (int64_t)blockIdx.x * FILTER_TPB + wave * 64;
  for (int j = 0; j < 64; ++j) {
    const unsigned long long mj = __shfl(m, j);
    if (mj == 0) continue;   // wave-uniform
    const int64_t aj = __shfl(at, j);
    if ((mj >> lane) & 1ull)
      p.out[aj + __popcll(mj & ((1ull << lane) - 1ull))] = p.first_id + (word0 + j) * 64 + lane;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------


int filter_check_call(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int B,
                      int for_search) {
  if (!ix) {
    set_error("Filter failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_filters < 0 || (n_filters > 0 && !filters)) {
    set_error("Filter failed: %s", n_filters < 0 ? "negative n_filters" : "n_filters > 0 but filters is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (for_search == 1 && ix->opts.shard_count > 1) {
    set_error("Filter failed: a filtered search needs the whole index on the handle (opened with shard_count = %d): the "
              "probe scaling needs the global subset length; np_hip_filter_eval works on a shard, and the sharded entries "
              "(np_hip_search_batch_sharded_filtered and its kin) exchange the lengths over a communicator",
              ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_filters > 0 && ix->columns.empty()) {
    set_error("Filter failed: the handle has no columns (np_hip_index_set_columns)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  int32_t types[NP_MAX_COLUMNS];
  const int32_t n_cols = (int32_t)ix->columns.size();
  for (int32_t c = 0; c < n_cols; ++c) types[c] = ix->columns[c].type;
  char why[200];
  for (int32_t f = 0; f < n_filters; ++f)
    if (filter_check_program(&filters[f], f, types, n_cols, why, sizeof why) != 0) {
      set_error("Filter failed: %s", why);
      return NP_ERR_INVALID_ARGUMENT;
    }
  NP_TRY(match_check_text(ix, filters, n_filters));
  if (for_search) {
    if (B > 0 && n_filters > 0 && !query_filter) {
      set_error("Filter failed: n_filters > 0 but query_filter is NULL");
      return NP_ERR_INVALID_ARGUMENT;
    }
    for (int b = 0; query_filter && b < B; ++b)
      if (query_filter[b] < -1 || query_filter[b] >= n_filters) {
        set_error("Filter failed: query_filter[%d] = %d is not -1 or a filter below %d", b, query_filter[b], n_filters);
        return NP_ERR_INVALID_ARGUMENT;
      }
  }
  return NP_OK;
}

// One evaluation: the programs and tables in `scratch`, chunked passes, ids either into a resident CSR or staged to the host.
struct FilterRun {
  const DeviceIndex* ix;
  hipStream_t st;
  const np_filter* filters;
  int32_t n_filters;
  FilterPlan plan;
  int64_t n_dc = 1, n_fc = 1;          // document and filter chunks
  // regions of scratch
  np_filter_op* d_ops = nullptr;
  int32_t* d_op_begin = nullptr;
  int64_t* d_values = nullptr;
  int64_t* d_totals = nullptr;         // [n_filters][n_dc]
  int64_t* d_table = nullptr;          // [n_filters * n_dc + 1]
  unsigned long long* d_mask = nullptr;
  uint32_t* d_counts = nullptr;
  int64_t* d_base = nullptr;
  int64_t* d_stage = nullptr;          // staged ids [plan.filters][plan.docs] (host output only)
  uint32_t* d_match_bits = nullptr;    // the NP_F_MATCH leaves' bitmaps over codes, one per distinct (column, DFA)
  std::vector<int64_t> h_table;

  size_t program_bytes(int64_t* n_ops, int64_t* n_vals) const {
    int64_t o = 0, v = 0;
    for (int32_t f = 0; f < n_filters; ++f) {
      o += filters[f].n_ops;
      for (int i = 0; i < filters[f].n_ops; ++i)   // a MATCH leaf's table stays on the host: the device reads its bitmap
        if (filters[f].ops[i].op != NP_F_MATCH) v += std::max(filters[f].ops[i].n_values, 0);
    }
    *n_ops = o;
    *n_vals = v;
    return up256((size_t)o * sizeof(np_filter_op)) + up256((size_t)(n_filters + 1) * 4) + up256((size_t)std::max<int64_t>(v, 1) * 8);
  }

  // plan + reserve + upload of the programs.  `stage` = ids leave through a staging area (np_hip_filter_eval)
  int prepare(DevBuf& scratch, bool stage) {
    int64_t n_ops = 0, n_vals = 0;
    const size_t b_prog = program_bytes(&n_ops, &n_vals);
    std::vector<MatchJob> jobs;
    std::vector<int64_t> match_at;   // per MATCH op, in program order: its bitmap's first word
    int64_t match_words = 0, match_work = 0;
    NP_TRY(match_collect(ix, filters, n_filters, &jobs, &match_at, &match_words, &match_work));
    const size_t b_match = up256((size_t)match_words * 4) + up256((size_t)match_work);
    const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
    const int64_t all_blocks = std::max<int64_t>(1, (ix->n_docs + NP_FILTER_BLOCK_DOCS - 1) / NP_FILTER_BLOCK_DOCS);
    // the tables are sized for the worst chunking: one block per document chunk
    const size_t b_tab_max = 2 * up256((size_t)(n_filters * all_blocks + 1) * 8);
    if (!filter_plan(budget, (int64_t)(b_prog + b_match + b_tab_max + 4096), ix->n_docs, n_filters, stage, &plan)) {
      set_error("Filter failed: one filter over %lld documents does not fit the workspace budget of %lld bytes",
                (long long)NP_FILTER_BLOCK_DOCS, (long long)budget);
      return NP_ERR_OUT_OF_MEMORY;
    }
    plan.filters = std::min<int32_t>(plan.filters, 65535);   // a chunk's filters are the grid's y dimension
    n_dc = std::max<int64_t>(1, (ix->n_docs + plan.docs - 1) / plan.docs);
    n_fc = (n_filters + plan.filters - 1) / plan.filters;
    const int64_t blocks = plan.blocks();
    const size_t b_tot = up256((size_t)(n_filters * n_dc) * 8), b_tab = up256((size_t)(n_filters * n_dc + 1) * 8);
    const size_t b_mask = up256((size_t)plan.filters * blocks * FILTER_TPB * 8), b_cnt = up256((size_t)plan.filters * blocks * 4),
                 b_base = up256((size_t)plan.filters * blocks * 8);
    const size_t b_stage = stage ? up256((size_t)plan.filters * plan.docs * 8) : 0;
    NP_TRY(scratch.reserve(b_prog + b_tot + b_tab + b_mask + b_cnt + b_base + b_stage + b_match));
    Carver carve{scratch.as<char>()};
    d_ops = (np_filter_op*)carve.take((size_t)n_ops * sizeof(np_filter_op));
    d_op_begin = (int32_t*)carve.take((size_t)(n_filters + 1) * 4);
    d_values = (int64_t*)carve.take((size_t)std::max<int64_t>(n_vals, 1) * 8);
    d_totals = (int64_t*)carve.take(b_tot);
    d_table = (int64_t*)carve.take(b_tab);
    d_mask = (unsigned long long*)carve.take(b_mask);
    d_counts = (uint32_t*)carve.take(b_cnt);
    d_base = (int64_t*)carve.take(b_base);
    d_stage = stage ? (int64_t*)carve.take(b_stage) : nullptr;
    d_match_bits = (uint32_t*)carve.take((size_t)match_words * 4);
    char* d_match_work = carve.take((size_t)match_work);
    // the programs, with every op's constants copied behind one another and its first_value re-based to them
    std::vector<np_filter_op> ops((size_t)n_ops);
    std::vector<int32_t> begin((size_t)n_filters + 1);
    std::vector<int64_t> vals((size_t)n_vals);
    int64_t o = 0, v = 0;
    size_t m = 0;
    for (int32_t f = 0; f < n_filters; ++f) {
      begin[f] = (int32_t)o;
      for (int i = 0; i < filters[f].n_ops; ++i) {
        ops[o] = filters[f].ops[i];
        if (ops[o].op == NP_F_MATCH) {
          ops[o].first_value = match_at[m++];   // the leaf reads the bitmap, not the table
        } else if (ops[o].n_values > 0) {
          memcpy(vals.data() + v, filters[f].values + ops[o].first_value, (size_t)ops[o].n_values * 8);
          ops[o].first_value = v;
          v += ops[o].n_values;
        } else {
          ops[o].first_value = 0;
        }
        ++o;
      }
    }
    begin[n_filters] = (int32_t)o;
    // pageable sources: the copies complete before the vectors go out of scope
    NP_HIP(hipMemcpyAsync(d_ops, ops.data(), (size_t)n_ops * sizeof(np_filter_op), hipMemcpyHostToDevice, st));
    NP_HIP(hipMemcpyAsync(d_op_begin, begin.data(), begin.size() * 4, hipMemcpyHostToDevice, st));
    if (n_vals > 0) NP_HIP(hipMemcpyAsync(d_values, vals.data(), (size_t)n_vals * 8, hipMemcpyHostToDevice, st));
    NP_HIP(hipStreamSynchronize(st));
    NP_TRY(match_run_jobs(ix, st, jobs, d_match_bits, d_match_work));
    return NP_OK;
  }

  // masks, block counts, block bases and the chunk's totals of filters [f0, f0 + nf) over document chunk dc
  int chunk_masks(int32_t f0, int32_t nf, int64_t dc) {
    const int64_t d0 = dc * plan.docs, n = std::min(plan.docs, ix->n_docs - d0), blocks = plan.blocks();
    const int64_t nw = blocks * FILTER_TPB, n_words = (n + 63) / 64;
    FilterEvalP p{ix->d_coltab.get(), d_ops, d_op_begin, d_values, f0, d0, n, nw, d_mask, d_match_bits};
    filter_mask_kernel<<<dim3((unsigned)((n + FILTER_TPB - 1) / FILTER_TPB), (unsigned)nf), FILTER_TPB, 0, st>>>(p);
    // every block of the plan is counted (words past n_words count 0): the scan reads `blocks` counts per filter
    filter_count_kernel<<<dim3((unsigned)blocks, (unsigned)nf), FILTER_TPB, 0, st>>>(d_mask, nw, n_words, blocks, d_counts);
    filter_scan_kernel<<<(unsigned)nf, FILTER_TPB, 0, st>>>(d_counts, blocks, d_base, d_totals, (int64_t)f0 * n_dc + dc, n_dc);
    NP_HIP(hipGetLastError());
    return NP_OK;
  }

  int chunk_compact(int32_t f0, int32_t nf, int64_t dc, int64_t* d_out, bool by_table) {
    const int64_t d0 = dc * plan.docs, n = std::min(plan.docs, ix->n_docs - d0), blocks = plan.blocks();
    const int64_t used_blocks = (n + NP_FILTER_BLOCK_DOCS - 1) / NP_FILTER_BLOCK_DOCS;
    FilterCompactP p{d_mask, d_base, by_table ? d_table : nullptr, (int64_t)f0 * n_dc + dc, n_dc, plan.docs,
                     blocks * FILTER_TPB, (n + 63) / 64, blocks, ix->doc_begin + d0, d_out};
    filter_compact_kernel<<<dim3((unsigned)used_blocks, (unsigned)nf), FILTER_TPB, 0, st>>>(p);
    NP_HIP(hipGetLastError());
    return NP_OK;
  }

  // pass 1: every chunk's totals, the table, and its host copy (synchronises)
  int count_all() {
    if (ix->n_docs > 0) {
      for (int64_t fc = 0; fc < n_fc; ++fc)
        for (int64_t dc = 0; dc < n_dc; ++dc) {
          const int32_t f0 = (int32_t)(fc * plan.filters);
          NP_TRY(chunk_masks(f0, std::min(plan.filters, n_filters - f0), dc));
        }
    } else {
      NP_HIP(hipMemsetAsync(d_totals, 0, (size_t)(n_filters * n_dc) * 8, st));
    }
    filter_table_kernel<<<1, FILTER_TPB, 0, st>>>(d_totals, n_filters * n_dc, d_table);
    NP_HIP(hipGetLastError());
    h_table.resize((size_t)(n_filters * n_dc + 1));
    NP_HIP(hipMemcpyAsync(h_table.data(), d_table, h_table.size() * 8, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    return NP_OK;
  }
  bool one_chunk() const { return n_fc == 1 && n_dc == 1; }   // the masks of pass 1 are still there
  int64_t offset(int32_t f) const { return h_table[(size_t)f * n_dc]; }
};

int filter_eval_resident(const DeviceIndex* ix, hipStream_t st, DevBuf& scratch, DevBuf& out, const np_filter* filters,
                         int32_t n_filters, const int32_t* h_query_filter, int B, FilterCsr* csr) {
  const auto t0 = std::chrono::steady_clock::now();
  FilterRun run{ix, st, filters, n_filters};
  NP_TRY(run.prepare(scratch, false));
  NP_TRY(run.count_all());
  csr->h_off.resize((size_t)n_filters + 1);
  for (int32_t f = 0; f <= n_filters; ++f) csr->h_off[f] = f < n_filters ? run.offset(f) : run.h_table.back();
  const int64_t total = csr->h_off[n_filters];
  const size_t b_ids = up256((size_t)std::max<int64_t>(total, 1) * 8), b_off = up256((size_t)(n_filters + 1) * 8);
  NP_TRY(out.reserve(b_ids + b_off + up256((size_t)std::max(B, 1) * 4)));
  char* base = out.as<char>();
  if (total > 0)
    for (int64_t fc = 0; fc < run.n_fc; ++fc)
      for (int64_t dc = 0; dc < run.n_dc; ++dc) {
        const int32_t f0 = (int32_t)(fc * run.plan.filters), nf = std::min(run.plan.filters, n_filters - f0);
        if (!run.one_chunk()) NP_TRY(run.chunk_masks(f0, nf, dc));
        NP_TRY(run.chunk_compact(f0, nf, dc, (int64_t*)base, true));
      }
  NP_HIP(hipMemcpyAsync(base + b_ids, csr->h_off.data(), (size_t)(n_filters + 1) * 8, hipMemcpyHostToDevice, st));
  if (B > 0) NP_HIP(hipMemcpyAsync(base + b_ids + b_off, h_query_filter, (size_t)B * 4, hipMemcpyHostToDevice, st));
  NP_HIP(hipStreamSynchronize(st));
  csr->d_ids = (const int64_t*)base;
  csr->d_off = (const int64_t*)(base + b_ids);
  csr->d_qsub = (const int32_t*)(base + b_ids + b_off);
  csr->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_filter_eval(const np_index* ix, const np_filter* filters, int32_t n_filters, int64_t* out_ids, int64_t ids_capacity,
                       int64_t* out_offsets) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  NP_TRY(filter_check_call(ix, filters, n_filters, nullptr, 0, false));
  if (!out_offsets) {
    set_error("Filter failed: out_offsets is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  out_offsets[0] = 0;
  if (n_filters == 0) return NP_OK;
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  FilterRun run{ix, use.stream, filters, n_filters};
  NP_TRY(run.prepare(use.filter_scratch(), out_ids != nullptr));
  NP_TRY(run.count_all());
  for (int32_t f = 0; f <= n_filters; ++f) out_offsets[f] = f < n_filters ? run.offset(f) : run.h_table.back();
  const int64_t total = out_offsets[n_filters];
  if (!out_ids || total == 0) return NP_OK;
  if (ids_capacity < total) {
    set_error("Filter failed: the filters select %lld ids, ids_capacity is %lld", (long long)total, (long long)ids_capacity);
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t fc = 0; fc < run.n_fc; ++fc)
    for (int64_t dc = 0; dc < run.n_dc; ++dc) {
      const int32_t f0 = (int32_t)(fc * run.plan.filters), nf = std::min(run.plan.filters, n_filters - f0);
      if (!run.one_chunk()) NP_TRY(run.chunk_masks(f0, nf, dc));
      NP_TRY(run.chunk_compact(f0, nf, dc, run.d_stage, false));
      for (int32_t f = f0; f < f0 + nf; ++f) {
        const int64_t at = run.h_table[(size_t)f * run.n_dc + dc], cnt = run.h_table[(size_t)f * run.n_dc + dc + 1] - at;
        if (cnt > 0)
          NP_HIP(hipMemcpyAsync(out_ids + at, run.d_stage + (int64_t)(f - f0) * run.plan.docs, (size_t)cnt * 8,
                                hipMemcpyDeviceToHost, use.stream));
      }
      NP_HIP(hipStreamSynchronize(use.stream));   // the staging area is reused by the next chunk
    }
  return NP_OK;
}

}  // extern "C"
