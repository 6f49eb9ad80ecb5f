// np_textmerge.hip -- keeping the device keyword index current (include/nextplaid_hip.h, "Merging keyword indexes"; DESIGN.md
// section 4): from a base index A, a verdict per old document (remap) and the index B of a batch of new texts, the index of
// the resulting table.  The host unites the two sorted vocabularies and finds, per batch document, where it falls among the
// old ids (np_textmerge_plan.h).  On the device every instance computes its own destination out of two scans and one
// logarithmic search over a run of the other side: no output atomics, no workgroup waits for another, integer arithmetic
// only, and the bytes are a function of the inputs alone.
#include <new>
#include "np_textbuild_dev.h"
#include "np_textmerge_plan.h"
#include "np_textres_plan.h"

namespace np {
namespace {

// first index in [0, n) whose entry is > v (n if none)
__device__ __forceinline__ int64_t tm_upper(const int64_t* __restrict__ a, int64_t n, int64_t v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// keep[i] = the document of A's instance i stays
__global__ void tm_keep(const int64_t* __restrict__ doc_a, const int64_t* __restrict__ remap, int64_t n_a, uint32_t* keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_a) keep[i] = remap[doc_a[i]] >= 0 ? 1u : 0u;
}

// per union term: the instances it keeps from A plus those it gets from B, and whether any is left
__global__ void tm_count(const int32_t* __restrict__ a_of, const int32_t* __restrict__ b_of, int64_t n_union,
                         const int64_t* __restrict__ toff_a, const int64_t* __restrict__ toff_b, const uint32_t* __restrict__ S,
                         uint32_t* cnt, uint32_t* alive) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n_union) return;
  const int32_t a = a_of[u], b = b_of[u];
  uint32_t c = 0;
  if (a >= 0) c += S[toff_a[a + 1]] - S[toff_a[a]];
  if (b >= 0) c += (uint32_t)(toff_b[b + 1] - toff_b[b]);
  cnt[u] = c;
  alive[u] = c > 0 ? 1u : 0u;
}

// A kept instance i of term a goes behind the kept instances of its run before it and behind the batch instances of the
// term whose new id is lower than its own.
__global__ void tm_place_a(const int64_t* __restrict__ toff_a, int64_t n_a_terms, const int64_t* __restrict__ doc_a,
                           const int32_t* __restrict__ pos_a, int64_t n_a, const int64_t* __restrict__ remap,
                           const uint32_t* __restrict__ keep, const uint32_t* __restrict__ S, const uint32_t* __restrict__ ua,
                           const int32_t* __restrict__ b_of, const int64_t* __restrict__ toff_b, const int64_t* __restrict__ doc_b,
                           const int64_t* __restrict__ delta_ids, const int64_t* __restrict__ off, int64_t total, int64_t* out_doc,
                           int32_t* out_pos) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_a || !keep[i]) return;
  const int64_t a = tm_upper(toff_a, n_a_terms + 1, i) - 1;   // the run that holds i; empty runs are stepped over
  const uint32_t u = ua[a];
  const int64_t nid = remap[doc_a[i]];
  int64_t before = 0;
  const int32_t b = b_of[u];
  if (b >= 0) {
    int64_t lo = toff_b[b], hi = toff_b[b + 1];
    const int64_t first = lo;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (delta_ids[doc_b[mid]] < nid) lo = mid + 1;
      else hi = mid;
    }
    before = lo - first;
  }
  const int64_t dst = off[u] + (int64_t)(S[i] - S[toff_a[a]]) + before;
  if (dst < total) {   // always, for arguments that passed the checks
    out_doc[dst] = nid;
    out_pos[dst] = pos_a[i];
  }
}

// A batch instance k of term b goes behind the batch instances of its run before it and behind the kept instances of the
// term whose OLD id is below bound[its document]: old ids ascend along a run of A, removed ones included.
__global__ void tm_place_b(const int64_t* __restrict__ toff_b, int64_t n_b_terms, const int64_t* __restrict__ doc_b,
                           const int32_t* __restrict__ pos_b, int64_t n_b, const int64_t* __restrict__ delta_ids,
                           const int64_t* __restrict__ bound, const uint32_t* __restrict__ ub, const int32_t* __restrict__ a_of,
                           const int64_t* __restrict__ toff_a, const int64_t* __restrict__ doc_a, const uint32_t* __restrict__ S,
                           const int64_t* __restrict__ off, int64_t total, int64_t* out_doc, int32_t* out_pos) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_b) return;
  const int64_t b = tm_upper(toff_b, n_b_terms + 1, k) - 1;
  const uint32_t u = ub[b];
  const int64_t d = doc_b[k];
  int64_t kept_before = 0;
  const int32_t a = a_of[u];
  if (a >= 0) {
    int64_t lo = toff_a[a], hi = toff_a[a + 1];
    const int64_t first = lo, bd = bound[d];
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (doc_a[mid] < bd) lo = mid + 1;
      else hi = mid;
    }
    kept_before = (int64_t)(S[lo] - S[first]);
  }
  const int64_t dst = off[u] + (k - toff_b[b]) + kept_before;
  if (dst < total) {
    out_doc[dst] = delta_ids[d];
    out_pos[dst] = pos_b[k];
  }
}

// term_offsets of the alive terms, and the total behind the last
__global__ void tm_offsets(const uint32_t* __restrict__ alive, const uint32_t* __restrict__ rank, const int64_t* __restrict__ off,
                           int64_t n_union, int64_t* out_toff) {
  const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (u > n_union) return;
  if (u == n_union || alive[u]) out_toff[rank[u]] = off[u];
}

template <class T>
int tm_upload(DevPtr<T>& p, const T* src, int64_t n, int64_t pad, hipStream_t st) {
  NP_TRY(p.alloc((size_t)(n + pad)));
  if (n > 0) NP_HIP(hipMemcpyAsync(p.get(), src, (size_t)n * sizeof(T), hipMemcpyHostToDevice, st));
  return NP_OK;
}

template <class T>
int tm_alloc(DevPtr<T>& p, int64_t n) {
  return p.alloc((size_t)std::max<int64_t>(n, 1));
}

}  // namespace

int text_merge_impl(const char* entry, int device, const np_text_index* base, const TextMergeResident* res, const uint8_t* a_bytes,
                    const int64_t* a_tbo, const int64_t* remap, int64_t n_remap, const np_text_build* delta, const int64_t* delta_ids,
                    int64_t n_rows_out, const np_text_merge_opts* opts, np_text_build* R, np_text_merge_report* rep) {
  const auto t_all = Clock::now();
  auto t0 = t_all;
  // ---- the batch: where its arrays lie
  TextMergeDelta D;
  const bool upload_b = delta && delta->merged;
  std::vector<int64_t> h_doc_b;   // the batch's documents on the host: the check counts the distinct ones
  const int64_t* b_toff_host = nullptr;
  const int32_t* b_pos_host = nullptr;
  if (delta) {
    if (!delta->finalised) {
      set_error("%s: delta is not finalised: call np_hip_text_build_sizes on it first", entry);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (delta->consumed) {
      set_error("%s: delta is consumed: np_hip_index_set_text_build installed it and its instance arrays belong to that handle", entry);
      return NP_ERR_INVALID_ARGUMENT;
    }
    if (delta->device != device) {
      set_error(res ? "%s: delta was built on device %d, the index lies on device %d" : "%s: delta was built on device %d, the call names device %d",
                entry, delta->device, device);
      return NP_ERR_INVALID_ARGUMENT;
    }
    const std::vector<uint8_t>& tb = upload_b ? delta->out.term_bytes : delta->term_bytes;
    const std::vector<int64_t>& tbo = upload_b ? delta->out.term_byte_offsets : delta->term_byte_offsets;
    D.term_bytes = tb.data();
    D.term_byte_offsets = tbo.data();
    D.n_terms = (int64_t)tbo.size() - 1;
    D.n_inst = upload_b ? (int64_t)delta->out.inst_doc.size() : delta->n_inst;
    D.n_docs = delta->n_docs;
  }
  if (delta && D.n_inst > 0) {
    if (upload_b) {
      D.inst_doc = delta->out.inst_doc.data();
      b_toff_host = delta->out.term_offsets.data();
      b_pos_host = delta->out.inst_pos.data();
    } else {   // the arrays lie in HBM: the device is there; a copy is no launch
      NP_TRY(build_check_device(device));
      DeviceGuard g0(device);
      h_doc_b.resize((size_t)D.n_inst);
      NP_HIP(hipMemcpy(h_doc_b.data(), delta->d_inst_doc.get(), (size_t)D.n_inst * 8, hipMemcpyDeviceToHost));
      D.inst_doc = h_doc_b.data();
    }
  } else if (upload_b) {
    b_toff_host = delta->out.term_offsets.data();
  }
  // ---- every check, with or without a device
  TextMergePlan P;
  char why[320];
  bool need_distinct = false;   // (resident base) the survivors that hold a token are counted on the device
  {
    int rc;
    if (res) {
      TextResBase hb;
      hb.present = res->ix->text.present;
      hb.shard_count = res->ix->opts.shard_count > 1 || res->ix->text.slice ? std::max(res->ix->opts.shard_count, 2) : 1;
      hb.n_terms = res->ix->text.n_terms;
      hb.n_inst = res->ix->text.n_inst;
      hb.n_docs = res->n_docs;
      rc = textres_merge_plan(hb, a_bytes, a_tbo, remap, n_remap, D, delta_ids, n_rows_out, upload_b || !delta,
                              opts ? opts->workspace_bytes : 0, &P, &need_distinct, why, sizeof(why));
    } else {
      rc = textmerge_plan(base, a_bytes, a_tbo, remap, n_remap, D, delta_ids, n_rows_out, upload_b || !delta,
                          opts ? opts->workspace_bytes : 0, &P, why, sizeof(why));
    }
    if (rc != NP_OK) {
      if (rc == NP_ERR_SHAPE) set_error("%s", why);
      else set_error("%s: %s", entry, why);
      return rc;
    }
  }
  NP_TRY(build_check_device(device));
  DeviceGuard g(device);
  if (!opts || opts->workspace_bytes == 0) {
    size_t free_b = 0, total_b = 0;
    NP_HIP(hipMemGetInfo(&free_b, &total_b));
    if (P.workspace_bytes > (int64_t)(free_b - free_b / 16)) {
      set_error("%s: the device's free memory of %zu bytes does not hold the call: it needs %lld", entry, free_b,
                (long long)P.workspace_bytes);
      return NP_ERR_OUT_OF_MEMORY;
    }
  }
  const double ms_check = ms_since(t0);

  // ---- upload
  t0 = Clock::now();
  TbStream Sx;
  NP_HIP(hipStreamCreateWithFlags(&Sx.st, hipStreamNonBlocking));
  hipStream_t st = Sx.st;
  const int64_t Ta = P.n_a_terms, Tb = P.n_b_terms, U = P.n_union, na = P.n_a, nb = P.n_b, m = P.n_delta_docs;
  DevPtr<int64_t> d_toff_a, d_doc_a, d_remap, d_ids, d_bound, d_off, ub_toff, ub_doc;
  DevPtr<int32_t> d_pos_a, d_a_of, d_b_of, ub_pos;
  DevPtr<uint32_t> d_keep, d_S, d_ua, d_ub, d_cnt, d_alive, d_rank;
  DevPtr<uint64_t> d_sums;
  const int64_t zero = 0;
  const int32_t* pos_a = nullptr;
  if (res) {   // the base is read where it lies: term_offsets and inst_doc regenerated from the postings, pos as it is
    NP_TRY(tm_alloc(d_toff_a, Ta + 1));
    NP_TRY(tm_alloc(d_doc_a, na + 1));
    NP_TRY(textres_expand(st, res->ix->text, d_toff_a.get(), d_doc_a.get()));
    pos_a = res->ix->text.pos.get();
  } else {
    NP_TRY(tm_upload(d_toff_a, Ta > 0 ? base->term_offsets : &zero, Ta + 1, 0, st));
    NP_TRY(tm_upload(d_doc_a, base->inst_doc, na, 1, st));
    NP_TRY(tm_upload(d_pos_a, base->inst_pos, na, 1, st));
    pos_a = d_pos_a.get();
  }
  NP_TRY(tm_upload(d_remap, remap, n_remap, 1, st));
  NP_TRY(tm_upload(d_ua, (const uint32_t*)P.ua.data(), Ta, 1, st));
  NP_TRY(tm_upload(d_ub, (const uint32_t*)P.ub.data(), Tb, 1, st));
  NP_TRY(tm_upload(d_a_of, (const int32_t*)P.a_of.data(), U, 1, st));
  NP_TRY(tm_upload(d_b_of, (const int32_t*)P.b_of.data(), U, 1, st));
  NP_TRY(tm_upload(d_ids, delta_ids, m, 1, st));
  NP_TRY(tm_upload(d_bound, (const int64_t*)P.bound.data(), m, 1, st));
  const int64_t *toff_b = nullptr, *doc_b = nullptr;
  const int32_t* pos_b = nullptr;
  if (upload_b || !delta) {
    NP_TRY(tm_upload(ub_toff, b_toff_host ? b_toff_host : &zero, Tb + 1, 0, st));
    toff_b = ub_toff.get();
    if (upload_b) {
      NP_TRY(tm_upload(ub_doc, D.inst_doc, nb, 1, st));
      NP_TRY(tm_upload(ub_pos, b_pos_host, nb, 1, st));
      doc_b = ub_doc.get();
      pos_b = ub_pos.get();
    }
  } else {   // read where it lies
    toff_b = delta->d_toff.get();
    doc_b = delta->d_inst_doc.get();
    pos_b = delta->d_inst_pos.get();
  }
  NP_TRY(tm_alloc(d_keep, na + 1));
  NP_TRY(tm_alloc(d_S, na + 1));
  NP_TRY(tm_alloc(d_cnt, U + 1));
  NP_TRY(tm_alloc(d_alive, U + 1));
  NP_TRY(tm_alloc(d_off, U + 1));
  NP_TRY(tm_alloc(d_rank, U + 1));
  NP_TRY(tm_alloc(d_sums, textbuild_scan_sums(std::max(na, U) + 1)));
  NP_HIP(hipStreamSynchronize(st));
  // (resident base) the counts over the handle's documents belong to this stage too: ms_upload is taken behind them
  if (res && (need_distinct || n_remap < res->n_docs)) {
    DevPtr<uint32_t> d_flag, d_scan;
    DevPtr<uint64_t> d_fsums;
    NP_TRY(tm_alloc(d_flag, res->n_docs + 1));
    NP_TRY(tm_alloc(d_scan, res->n_docs + 1));
    NP_TRY(tm_alloc(d_fsums, textbuild_scan_sums(res->n_docs + 1)));
    const int32_t* doc_len = res->ix->text.doc_len.get();
    const int64_t n_told = std::min(n_remap, res->n_docs);   // the handle's documents that have a verdict
    if (n_told < res->n_docs) {   // a base document >= n_remap: the documents behind remap must hold no token
      int64_t beyond = 0;
      NP_TRY(textres_count_docs(st, doc_len + n_told, res->n_docs - n_told, nullptr, d_flag.get(), d_scan.get(), d_fsums.get(), &beyond));
      if (beyond > 0) {
        set_error("%s: base: %lld documents of the handle's keyword index hold a token and lie outside the index (the index is n_remap = "
                  "%lld old documents)", entry, (long long)beyond, (long long)n_remap);
        return NP_ERR_INVALID_ARGUMENT;
      }
    }
    if (need_distinct) {   // n_rows_out against the documents of the result that hold a token: the batch's plus the survivors'
      int64_t distinct = 0;
      NP_TRY(textres_count_docs(st, doc_len, n_told, d_remap.get(), d_flag.get(), d_scan.get(), d_fsums.get(), &distinct));
      std::vector<bool> seen_b((size_t)D.n_docs, false);
      for (int64_t k = 0; k < D.n_inst; ++k)
        if (!seen_b[(size_t)D.inst_doc[k]]) seen_b[(size_t)D.inst_doc[k]] = true, ++distinct;
      if (n_rows_out < distinct) {
        set_error("%s: n_rows_out %lld is below the %lld documents of the result that hold a token", entry, (long long)n_rows_out,
                  (long long)distinct);
        return NP_ERR_INVALID_ARGUMENT;
      }
    }
  }

  const double ms_upload = ms_since(t0);

  // ---- keep, S; the terms' counts, off and the alive terms' numbers
  t0 = Clock::now();
  if (na > 0) {
    hipLaunchKernelGGL(tm_keep, dim3(grid_of(na, 256)), dim3(256), 0, st, (const int64_t*)d_doc_a.get(), (const int64_t*)d_remap.get(), na,
                       d_keep.get());
    NP_HIP(hipGetLastError());
  }
  NP_TRY(tb_scan<uint32_t>(st, d_keep.get(), na, d_S.get(), d_sums.get()));
  if (U > 0) {
    hipLaunchKernelGGL(tm_count, dim3(grid_of(U, 256)), dim3(256), 0, st, (const int32_t*)d_a_of.get(), (const int32_t*)d_b_of.get(), U,
                       (const int64_t*)d_toff_a.get(), toff_b, (const uint32_t*)d_S.get(), d_cnt.get(), d_alive.get());
    NP_HIP(hipGetLastError());
  }
  NP_TRY(tb_scan<int64_t>(st, d_cnt.get(), U, d_off.get(), d_sums.get()));
  NP_TRY(tb_scan<uint32_t>(st, d_alive.get(), U, d_rank.get(), d_sums.get()));
  std::vector<uint32_t> h_alive((size_t)U);
  int64_t total = 0;
  uint32_t n_alive = 0;
  if (U > 0) NP_HIP(hipMemcpyAsync(h_alive.data(), d_alive.get(), (size_t)U * 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipMemcpyAsync(&total, d_off.get() + U, 8, hipMemcpyDeviceToHost, st));
  NP_HIP(hipMemcpyAsync(&n_alive, d_rank.get() + U, 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipStreamSynchronize(st));
  const double ms_count = ms_since(t0);
  if (total < 0 || total > na + nb || (int64_t)n_alive > U) {
    set_error("%s: the device counted %lld instances and %u terms from %lld + %lld instances and %lld terms", entry,
              (long long)total, n_alive, (long long)na, (long long)nb, (long long)U);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }

  // ---- the strings of the alive terms
  t0 = Clock::now();
  textmerge_compact_terms(P, h_alive.data(), a_bytes, a_tbo, D.term_bytes, D.term_byte_offsets, &R->term_bytes, &R->term_byte_offsets);
  const double ms_terms = ms_since(t0);

  // ---- place
  t0 = Clock::now();
  NP_TRY(tm_alloc(R->d_toff, (int64_t)n_alive + 1));
  NP_TRY(tm_alloc(R->d_inst_doc, total));
  NP_TRY(tm_alloc(R->d_inst_pos, total));
  if (na > 0 && total > 0) {
    hipLaunchKernelGGL(tm_place_a, dim3(grid_of(na, 256)), dim3(256), 0, st, (const int64_t*)d_toff_a.get(), Ta,
                       (const int64_t*)d_doc_a.get(), pos_a, na, (const int64_t*)d_remap.get(),
                       (const uint32_t*)d_keep.get(), (const uint32_t*)d_S.get(), (const uint32_t*)d_ua.get(), (const int32_t*)d_b_of.get(),
                       toff_b, doc_b, (const int64_t*)d_ids.get(), (const int64_t*)d_off.get(), total, R->d_inst_doc.get(),
                       R->d_inst_pos.get());
    NP_HIP(hipGetLastError());
  }
  if (nb > 0) {
    hipLaunchKernelGGL(tm_place_b, dim3(grid_of(nb, 256)), dim3(256), 0, st, toff_b, Tb, doc_b, pos_b, nb, (const int64_t*)d_ids.get(),
                       (const int64_t*)d_bound.get(), (const uint32_t*)d_ub.get(), (const int32_t*)d_a_of.get(),
                       (const int64_t*)d_toff_a.get(), (const int64_t*)d_doc_a.get(), (const uint32_t*)d_S.get(),
                       (const int64_t*)d_off.get(), total, R->d_inst_doc.get(), R->d_inst_pos.get());
    NP_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(tm_offsets, dim3(grid_of(U + 1, 256)), dim3(256), 0, st, (const uint32_t*)d_alive.get(), (const uint32_t*)d_rank.get(),
                     (const int64_t*)d_off.get(), U, R->d_toff.get());
  NP_HIP(hipGetLastError());
  NP_HIP(hipStreamSynchronize(st));
  const double ms_place = ms_since(t0);

  R->device = device;
  R->tokenizer = delta ? delta->tokenizer : 0;
  R->n_docs = n_rows_out;   // what np_hip_text_build_sizes reports as n_rows
  R->n_inst = total;
  R->n_terms = (int64_t)n_alive;
  R->finalised = true;      // nothing may be added to a merge's result
  if (rep) {
    memset(rep, 0, sizeof(*rep));
    rep->n_base_terms = Ta;
    rep->n_base_instances = na;
    rep->n_old_docs = n_remap;
    rep->n_survivors = P.n_survivors;
    rep->n_delta_docs = m;
    rep->n_delta_terms = Tb;
    rep->n_delta_instances = nb;
    rep->n_terms = (int64_t)n_alive;
    rep->n_instances = total;
    rep->n_rows = n_rows_out;
    rep->n_terms_dropped = U - (int64_t)n_alive;
    rep->n_instances_dropped = na + nb - total;
    rep->delta_uploaded = upload_b || !delta ? 1 : 0;
    rep->ms_check = ms_check;
    rep->ms_upload = ms_upload;
    rep->ms_count = ms_count;
    rep->ms_terms = ms_terms;
    rep->ms_place = ms_place;
    rep->ms_total = ms_since(t_all);
    rep->workspace_bytes = P.workspace_bytes;
  }
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" int np_hip_text_build_merge(int32_t device, const np_text_index* base, const uint8_t* base_term_bytes,
                                       const int64_t* base_term_byte_offsets, const int64_t* remap, int64_t n_remap,
                                       const np_text_build* delta, const int64_t* delta_ids, int64_t n_rows_out,
                                       const np_text_merge_opts* opts, np_text_build** out_build, np_text_merge_report* report) {
  clear_error();
  if (!out_build) {
    set_error("np_hip_text_build_merge: out_build is NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out_build = nullptr;
  np_text_build* b = new (std::nothrow) np_text_build();
  if (!b) {
    set_error("np_hip_text_build_merge: out of host memory");
    return NP_ERR_OUT_OF_MEMORY;
  }
  int rc;
  try {
    rc = text_merge_impl("np_hip_text_build_merge", device, base, nullptr, base_term_bytes, base_term_byte_offsets, remap, n_remap, delta, delta_ids, n_rows_out, opts, b,
                         report);
  } catch (const std::bad_alloc&) {
    set_error("np_hip_text_build_merge: out of host memory");
    rc = NP_ERR_OUT_OF_MEMORY;
  }
  if (rc != NP_OK) {
    np_hip_text_build_free(b);
    return rc;
  }
  *out_build = b;
  return NP_OK;
}
