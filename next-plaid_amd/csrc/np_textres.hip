// np_textres.hip -- the handle's keyword index built and updated without leaving HBM (include/nextplaid_hip.h, "The resident
// keyword index"): np_hip_index_set_text_build derives the postings of a finalised device build by
// kernels and takes the build's positions as they lie; np_hip_index_text_merge is np_hip_text_build_merge whose base is the
// handle's keyword index, its term_offsets and inst_doc regenerated from the postings by one expanding launch; and the
// read-back of the index, as a table and as it lies.  No workgroup waits for another; the only atomics are integer adds into
// doc_len, whose sum does not depend on the order they arrive in; the arithmetic is integers only, so the bytes are a
// function of the inputs alone.
#include <new>
#include "np_textbuild_dev.h"
#include "np_textres_plan.h"

namespace np {
namespace {

constexpr int64_t NO_OFFENDER = INT64_MAX;

// flag[toff[k]] = 1 for every term that holds an instance (flag is zeroed before)
__global__ void tr_mark(const int64_t* __restrict__ toff, int64_t n_terms, int64_t n, uint32_t* flag) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_terms) return;
  const int64_t at = toff[k];
  if (at < toff[k + 1] && at >= 0 && at < n) flag[at] = 1u;   // (inside for every build the library made)
}

// Per instance: the verdict of np_hip_index_set_text's checks, and whether it starts a posting -- the first of its term
// (flag, as tr_mark left it) or another document than its predecessor's.  In place: lane i reads flag[i] alone.  bad[block] =
// the lowest offending instance of the block's NP_TR_CHUNK instances.
__global__ __launch_bounds__(256) void tr_check_heads(const int64_t* __restrict__ doc, const int32_t* __restrict__ pos, int64_t n,
                                                       int64_t n_docs, uint32_t* flag, int64_t* bad) {
  __shared__ int64_t lds[256];
  const int64_t i0 = (int64_t)blockIdx.x * NP_TR_CHUNK + threadIdx.x * 8;
  int64_t low = NO_OFFENDER;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int64_t i = i0 + j;
    if (i >= n) break;
    const bool first = flag[i] != 0u || i == 0;
    const int64_t d = doc[i], pd = first ? 0 : doc[i - 1];
    const int32_t pp = first ? 0 : pos[i - 1];
    if (textres_rule(d, pos[i], first, pd, pp, n_docs) != 0 && low == NO_OFFENDER) low = i;
    flag[i] = (first || pd != d) ? 1u : 0u;
  }
  lds[threadIdx.x] = low;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] = min(lds[threadIdx.x], lds[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) bad[blockIdx.x] = lds[0];
}

// at a head: the posting's document and its first instance
__global__ void tr_postings(const int64_t* __restrict__ doc, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank,
                            int64_t n, int64_t n_post, int32_t* post_doc, int64_t* post_first) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !head[i]) return;
  const int64_t p = rank[i];
  if (p < n_post) {   // always: rank is the scan of head
    post_doc[p] = (int32_t)doc[i];
    post_first[p] = i;
  }
}

// a posting's term frequency is the distance to the next head; the document's length gains it
__global__ void tr_tf(const int64_t* __restrict__ post_first, const int32_t* __restrict__ post_doc, int64_t n_post, int64_t n,
                      int64_t n_docs, int32_t* post_tf, int32_t* doc_len) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_post) return;
  const int32_t tf = (int32_t)((p + 1 < n_post ? post_first[p + 1] : n) - post_first[p]);
  post_tf[p] = tf;
  const int32_t d = post_doc[p];
  if (d >= 0 && d < n_docs) atomicAdd(&doc_len[d], tf);   // (always inside: the check passed)
}

// post_off[k] = the postings before term k's first instance; rank[n] = n_post closes the last list
__global__ void tr_post_off(const int64_t* __restrict__ toff, const uint32_t* __restrict__ rank, int64_t n_terms, int64_t n,
                            int64_t* post_off) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_terms) return;
  const int64_t at = toff[k];
  post_off[k] = rank[at < 0 ? 0 : (at < n ? at : n)];
}

// flag[d] = document d holds a token (and, with remap, stays)
__global__ void tr_doc_flags(const int32_t* __restrict__ doc_len, int64_t n_docs, const int64_t* __restrict__ remap, uint32_t* flag) {
  const int64_t d = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d < n_docs) flag[d] = (doc_len[d] > 0 && (!remap || remap[d] >= 0)) ? 1u : 0u;
}

// term_offsets from the postings: a term's first instance is its first posting's; a term without postings starts where the
// next one does
__global__ void tr_expand_toff(const int64_t* __restrict__ post_off, const int64_t* __restrict__ post_first, int64_t n_terms,
                               int64_t n_post, int64_t n_inst, int64_t* toff) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k > n_terms) return;
  const int64_t po = post_off[k];
  toff[k] = (po >= 0 && po < n_post) ? post_first[po] : n_inst;
}

// an instance's document is that of the posting whose [post_first, post_first + tf) holds it: the last posting that starts
// at or before it
__global__ void tr_expand_doc(const int64_t* __restrict__ post_first, const int32_t* __restrict__ post_doc, int64_t n_post,
                              int64_t n_inst, int64_t* inst_doc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_inst) return;
  int64_t lo = 0, hi = n_post;   // first posting that starts behind i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (post_first[mid] <= i) lo = mid + 1;
    else hi = mid;
  }
  inst_doc[i] = lo > 0 ? (int64_t)post_doc[lo - 1] : 0;
}

template <class T>
int tr_alloc(DevPtr<T>& p, int64_t n, size_t* acct = nullptr) {
  return p.alloc((size_t)std::max<int64_t>(n, 1), acct);
}

// The install's allocations against its plan: every array the call allocates or is handed, rounded as the plan rounds.
struct TrHeld {
  int64_t bytes = 0;
  template <class T>
  int take(DevPtr<T>& p, int64_t n, size_t* acct = nullptr) {
    bytes += textbuild_up256(std::max<int64_t>(n, 1) * (int64_t)sizeof(T));
    return tr_alloc(p, n, acct);
  }
  void handed(int64_t b) { bytes += textbuild_up256(b); }
};

int check_free_memory(const char* entry, int64_t need) {
  size_t free_b = 0, total_b = 0;
  NP_HIP(hipMemGetInfo(&free_b, &total_b));
  if (need > (int64_t)(free_b - free_b / 16)) {
    set_error("%s: the device's free memory of %zu bytes does not hold the call: it needs %lld", entry, free_b, (long long)need);
    return NP_ERR_OUT_OF_MEMORY;
  }
  return NP_OK;
}

// The lowest offender named as np_hip_index_set_text names it: its rule from the same function the kernel ran, its term from
// the term starts.
int name_offender(const char* entry, int64_t inst, const int64_t* d_toff, int64_t n_terms, const int64_t* d_doc, const int32_t* d_pos,
                  int64_t n_docs) {
  std::vector<int64_t> toff((size_t)n_terms + 1);
  NP_HIP(hipMemcpy(toff.data(), d_toff, toff.size() * 8, hipMemcpyDeviceToHost));
  const int64_t term = (int64_t)(std::upper_bound(toff.begin(), toff.end(), inst) - toff.begin()) - 1;
  const bool first = term >= 0 && toff[(size_t)term] == inst;
  int64_t d[2] = {0, 0};
  int32_t p[2] = {0, 0};
  const int64_t from = first || inst == 0 ? inst : inst - 1, cnt = inst - from + 1;
  NP_HIP(hipMemcpy(d + (2 - cnt), d_doc + from, (size_t)cnt * 8, hipMemcpyDeviceToHost));
  NP_HIP(hipMemcpy(p + (2 - cnt), d_pos + from, (size_t)cnt * 4, hipMemcpyDeviceToHost));
  const int rule = textres_rule(d[1], p[1], first || inst == 0, d[0], p[0], n_docs);
  char why[240];
  textres_offender_message(rule, inst, term, d[1], p[1], why, sizeof(why));
  set_error("%s: %s", entry, why);
  return NP_ERR_INVALID_ARGUMENT;
}

const char* const kInstall = "np_hip_index_set_text_build";

int install_impl(DeviceIndex* ix, np_text_build* B) {
  const bool uploaded = B->merged;
  const int64_t T = uploaded ? B->out.n_terms() : B->n_terms;
  const int64_t n = uploaded ? (int64_t)B->out.inst_doc.size() : B->n_inst;
  const int64_t n_rows = B->n_docs, n_docs = ix->n_docs;
  const int64_t need = textres_install_bytes(T, n, n_docs);
  DeviceText fresh;
  size_t bytes = 0;
  int64_t n_post = 0;
  TrHeld H;
  if (!(n == 0 && n_rows == 0)) {   // (an index without instances and rows drops what the handle had, as np_hip_index_set_text)
    // the arrays the call allocates: everything planned but the build's own three, where they lie in HBM already
    NP_TRY(check_free_memory(kInstall, uploaded ? need : need - textbuild_up256((T + 1) * 8) - textbuild_up256(n * 8 + 8) -
                                                             textbuild_up256(n * 4 + 4)));
    TbStream Sx;
    NP_HIP(hipStreamCreateWithFlags(&Sx.st, hipStreamNonBlocking));
    hipStream_t st = Sx.st;
    DevPtr<int64_t> up_toff, up_doc;
    DevPtr<int32_t> up_pos;
    if (uploaded) {   // a build that np_hip_text_build_sizes merged on the host: its arrays lie in `out`
      NP_TRY(H.take(up_toff, T + 1));
      NP_TRY(H.take(up_doc, n));
      NP_TRY(H.take(up_pos, n));
      NP_HIP(hipMemcpyAsync(up_toff.get(), B->out.term_offsets.data(), (size_t)(T + 1) * 8, hipMemcpyHostToDevice, st));
      if (n > 0) {
        NP_HIP(hipMemcpyAsync(up_doc.get(), B->out.inst_doc.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
        NP_HIP(hipMemcpyAsync(up_pos.get(), B->out.inst_pos.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
      }
    }
    if (!uploaded) {   // the build's own three arrays, which the call is handed
      H.handed((T + 1) * 8);
      H.handed(n * 8 + 8);
      H.handed(n * 4 + 4);
    }
    const int64_t* toff = uploaded ? up_toff.get() : B->d_toff.get();
    const int64_t* doc = uploaded ? up_doc.get() : B->d_inst_doc.get();
    const int32_t* pos = uploaded ? up_pos.get() : B->d_inst_pos.get();
    const int64_t m = std::max(n, n_docs) + 1, nblk = textres_blocks(n);
    DevPtr<uint32_t> d_flag, d_rank;
    DevPtr<uint64_t> d_sums;
    DevPtr<int64_t> d_bad;
    NP_TRY(H.take(d_flag, m));
    NP_TRY(H.take(d_rank, m));
    NP_TRY(H.take(d_sums, textbuild_scan_sums(m)));
    NP_TRY(H.take(d_bad, nblk + 1));
    NP_TRY(H.take(fresh.doc_len, n_docs, &bytes));
    NP_TRY(H.take(fresh.post_off, T + 1, &bytes));
    NP_HIP(hipMemsetAsync(fresh.doc_len.get(), 0, (size_t)std::max<int64_t>(n_docs, 1) * 4, st));

    // ---- check and heads
    std::vector<int64_t> h_bad((size_t)nblk);
    if (n > 0) {
      NP_HIP(hipMemsetAsync(d_flag.get(), 0, (size_t)n * 4, st));
      if (T > 0) hipLaunchKernelGGL(tr_mark, dim3(grid_of(T, 256)), dim3(256), 0, st, toff, T, n, d_flag.get());
      hipLaunchKernelGGL(tr_check_heads, dim3((unsigned)nblk), dim3(256), 0, st, doc, pos, n, n_docs, d_flag.get(), d_bad.get());
      NP_HIP(hipGetLastError());
      NP_HIP(hipMemcpyAsync(h_bad.data(), d_bad.get(), (size_t)nblk * 8, hipMemcpyDeviceToHost, st));
    }
    NP_TRY(tb_scan<uint32_t>(st, d_flag.get(), n, d_rank.get(), d_sums.get()));
    uint32_t np32 = 0;
    NP_HIP(hipMemcpyAsync(&np32, d_rank.get() + n, 4, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    const int64_t low = h_bad.empty() ? NO_OFFENDER : *std::min_element(h_bad.begin(), h_bad.end());
    if (low != NO_OFFENDER) return name_offender(kInstall, low, toff, T, doc, pos, n_docs);
    n_post = (int64_t)np32;
    if (n_post > n) {
      set_error("%s: the device counted %lld postings from %lld instances", kInstall, (long long)n_post, (long long)n);
      return NP_ERR_DEVICE_UNAVAILABLE;
    }

    // ---- postings, term frequencies, document lengths, the terms' lists
    NP_TRY(H.take(fresh.post_doc, n_post, &bytes));
    NP_TRY(H.take(fresh.post_tf, n_post, &bytes));
    NP_TRY(H.take(fresh.post_first, n_post, &bytes));
    if (n > 0) {
      hipLaunchKernelGGL(tr_postings, dim3(grid_of(n, 256)), dim3(256), 0, st, doc, (const uint32_t*)d_flag.get(),
                         (const uint32_t*)d_rank.get(), n, n_post, fresh.post_doc.get(), fresh.post_first.get());
      hipLaunchKernelGGL(tr_tf, dim3(grid_of(n_post, 256)), dim3(256), 0, st, (const int64_t*)fresh.post_first.get(),
                         (const int32_t*)fresh.post_doc.get(), n_post, n, n_docs, fresh.post_tf.get(), fresh.doc_len.get());
    }
    hipLaunchKernelGGL(tr_post_off, dim3(grid_of(T + 1, 256)), dim3(256), 0, st, toff, (const uint32_t*)d_rank.get(), T, n,
                       fresh.post_off.get());
    NP_HIP(hipGetLastError());
    fresh.h_post_off.assign((size_t)T + 1, 0);
    NP_HIP(hipMemcpyAsync(fresh.h_post_off.data(), fresh.post_off.get(), (size_t)(T + 1) * 8, hipMemcpyDeviceToHost, st));
    // ---- n_rows against the documents that hold a token: the nonzero entries of doc_len (flag and rank are free again)
    uint32_t distinct = 0;
    if (n_docs > 0)
      hipLaunchKernelGGL(tr_doc_flags, dim3(grid_of(n_docs, 256)), dim3(256), 0, st, (const int32_t*)fresh.doc_len.get(), n_docs,
                         (const int64_t*)nullptr, d_flag.get());
    NP_TRY(tb_scan<uint32_t>(st, d_flag.get(), n_docs, d_rank.get(), d_sums.get()));
    NP_HIP(hipMemcpyAsync(&distinct, d_rank.get() + n_docs, 4, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    if (n_rows < (int64_t)distinct) {
      set_error("%s: build: n_rows = %lld is below the %lld documents that hold a token", kInstall, (long long)n_rows, (long long)distinct);
      return NP_ERR_INVALID_ARGUMENT;
    }

    if (H.bytes > need) {   // the plan is an upper bound of what the call held: anything else is a defect of the plan
      set_error("%s: the call held %lld bytes, its plan (np_hip_index_set_text_build_bytes) says %lld", kInstall, (long long)H.bytes,
                (long long)need);
      return NP_ERR_DEVICE_UNAVAILABLE;
    }
    // ---- the positions are inst_pos verbatim: the build's array changes its owner
    if (uploaded) fresh.pos = std::move(up_pos);
    else if (n > 0) fresh.pos = std::move(B->d_inst_pos);
    else NP_TRY(H.take(fresh.pos, 0));
    bytes += fresh.pos.bytes();
    fresh.n_terms = T;
    fresh.n_post = n_post;
    fresh.n_inst = n;
    fresh.n_rows = n_rows;
    fresh.total_tokens = n;
    fresh.slice = false;
    fresh.present = true;
  }
  // ---- the build is consumed: its sizes and vocabulary stay
  B->d_inst_doc.reset();
  B->d_inst_pos.reset();
  B->d_toff.reset();
  std::vector<int64_t>().swap(B->out.term_offsets);
  std::vector<int64_t>().swap(B->out.inst_doc);
  std::vector<int32_t>().swap(B->out.inst_pos);
  if (uploaded) B->n_inst = n;   // (np_hip_text_build_sizes read it from `out`)
  B->consumed = true;
  ix->text = std::move(fresh);   // frees the old index
  ix->device_bytes = ix->device_bytes - ix->text_bytes + bytes;
  ix->text_bytes = bytes;
  return NP_OK;
}

// the handle's keyword index as the read-back entries need it: whole, on an unsharded handle
int check_readable(const char* entry, const DeviceIndex* ix) {
  if (!ix) {
    set_error("%s: index is NULL", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->opts.shard_count > 1 || ix->text.slice) {
    set_error("%s: index is a shard (opened with shard_count = %d): a slice does not hold the whole table", entry, ix->opts.shard_count);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (!ix->text.present) {
    set_error("%s: index has no keyword index (np_hip_index_set_text, np_hip_index_set_text_build)", entry);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

}  // namespace

int textres_expand(hipStream_t st, const DeviceText& t, int64_t* toff, int64_t* inst_doc) {
  hipLaunchKernelGGL(tr_expand_toff, dim3(grid_of(t.n_terms + 1, 256)), dim3(256), 0, st, (const int64_t*)t.post_off.get(),
                     (const int64_t*)t.post_first.get(), t.n_terms, t.n_post, t.n_inst, toff);
  if (t.n_inst > 0)
    hipLaunchKernelGGL(tr_expand_doc, dim3(grid_of(t.n_inst, 256)), dim3(256), 0, st, (const int64_t*)t.post_first.get(),
                       (const int32_t*)t.post_doc.get(), t.n_post, t.n_inst, inst_doc);
  NP_HIP(hipGetLastError());
  return NP_OK;
}

int textres_count_docs(hipStream_t st, const int32_t* doc_len, int64_t n, const int64_t* d_remap, uint32_t* flags, uint32_t* scan,
                       uint64_t* sums, int64_t* out) {
  if (n > 0) hipLaunchKernelGGL(tr_doc_flags, dim3(grid_of(n, 256)), dim3(256), 0, st, doc_len, n, d_remap, flags);
  NP_TRY(tb_scan<uint32_t>(st, flags, n, scan, sums));
  uint32_t total = 0;
  NP_HIP(hipMemcpyAsync(&total, scan + n, 4, hipMemcpyDeviceToHost, st));
  NP_HIP(hipStreamSynchronize(st));
  *out = (int64_t)total;
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_index_set_text_build(np_index* ix, np_text_build* build) {
  clear_error();
  TextResInstall a;
  a.index_null = !ix;
  a.build_null = !build;
  if (ix) {
    a.index_device = ix->device;
    a.shard_count = ix->opts.shard_count;
    a.n_docs = ix->n_docs;
  }
  if (build) {
    a.finalised = build->finalised;
    a.consumed = build->consumed;
    a.build_device = build->device;
    a.n_terms = build->merged ? build->out.n_terms() : build->n_terms;
    a.n_inst = build->merged ? (int64_t)build->out.inst_doc.size() : build->n_inst;
    a.n_rows = build->n_docs;
  }
  char why[320];
  auto refuse = [&](int rc) {
    if (rc == NP_ERR_SHAPE) set_error("%s", why);
    else set_error("%s: %s", kInstall, why);
    return rc;
  };
  if (const int rc = textres_check_install(a, why, sizeof(why))) return refuse(rc);
  // the handle as np_hip_index_append takes it: running calls finish on the old keyword index, later ones see the new one
  HoldContexts hold(ix);
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  NP_HIP(hipDeviceSynchronize());   // device-side calls that returned may still read the old index on their streams
  try {
    return install_impl(ix, build);
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", kInstall);
    return NP_ERR_OUT_OF_MEMORY;
  }
}

int64_t np_hip_index_set_text_build_bytes(int64_t n_terms, int64_t n_instances, int64_t n_docs) {
  return textres_install_bytes(n_terms, n_instances, n_docs);
}

int np_hip_index_text_merge(const np_index* ix, const uint8_t* base_term_bytes, const int64_t* base_term_byte_offsets,
                            const int64_t* remap, int64_t n_remap, const np_text_build* delta, const int64_t* delta_ids,
                            int64_t n_rows_out, const np_text_merge_opts* opts, np_text_build** out_build,
                            np_text_merge_report* report) {
  static const char* const kMerge = "np_hip_index_text_merge";
  clear_error();
  if (!out_build) {
    set_error("%s: out_build is NULL", kMerge);
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out_build = nullptr;
  if (!ix) {
    set_error("%s: index is NULL", kMerge);
    return NP_ERR_INVALID_ARGUMENT;
  }
  IndexRead reading(ix);   // an append or an install waits for this call and holds later ones back (np_internal.h)
  np_text_build* b = new (std::nothrow) np_text_build();
  if (!b) {
    set_error("%s: out of host memory", kMerge);
    return NP_ERR_OUT_OF_MEMORY;
  }
  TextMergeResident res;
  res.ix = ix;
  res.n_docs = ix->n_docs;
  int rc;
  try {
    rc = text_merge_impl(kMerge, ix->device, nullptr, &res, base_term_bytes, base_term_byte_offsets, remap, n_remap, delta, delta_ids,
                         n_rows_out, opts, b, report);
  } catch (const std::bad_alloc&) {
    set_error("%s: out of host memory", kMerge);
    rc = NP_ERR_OUT_OF_MEMORY;
  }
  if (rc != NP_OK) {
    np_hip_text_build_free(b);
    return rc;
  }
  *out_build = b;
  return NP_OK;
}

int np_hip_index_text_sizes(const np_index* ix, int64_t* n_terms, int64_t* n_postings, int64_t* n_instances, int64_t* n_rows,
                            int64_t* n_docs) {
  clear_error();
  IndexRead reading(ix);
  NP_TRY(check_readable("np_hip_index_text_sizes", ix));
  if (n_terms) *n_terms = ix->text.n_terms;
  if (n_postings) *n_postings = ix->text.n_post;
  if (n_instances) *n_instances = ix->text.n_inst;
  if (n_rows) *n_rows = ix->text.n_rows;
  if (n_docs) *n_docs = ix->n_docs;
  return NP_OK;
}

int np_hip_index_get_text(const np_index* ix, int64_t* term_offsets, int64_t* inst_doc, int32_t* inst_pos) {
  clear_error();
  IndexRead reading(ix);
  NP_TRY(check_readable("np_hip_index_get_text", ix));
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  const DeviceText& t = ix->text;
  if (term_offsets || inst_doc) {
    TbStream Sx;
    NP_HIP(hipStreamCreateWithFlags(&Sx.st, hipStreamNonBlocking));
    DevPtr<int64_t> d_toff, d_doc;
    NP_TRY(tr_alloc(d_toff, t.n_terms + 1));
    NP_TRY(tr_alloc(d_doc, t.n_inst));
    NP_TRY(textres_expand(Sx.st, t, d_toff.get(), d_doc.get()));
    NP_HIP(hipStreamSynchronize(Sx.st));
    if (term_offsets) NP_HIP(hipMemcpy(term_offsets, d_toff.get(), (size_t)(t.n_terms + 1) * 8, hipMemcpyDeviceToHost));
    if (inst_doc && t.n_inst > 0) NP_HIP(hipMemcpy(inst_doc, d_doc.get(), (size_t)t.n_inst * 8, hipMemcpyDeviceToHost));
  }
  if (inst_pos && t.n_inst > 0) NP_HIP(hipMemcpy(inst_pos, t.pos.get(), (size_t)t.n_inst * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

int np_hip_index_get_text_layout(const np_index* ix, int64_t* post_off, int32_t* post_doc, int32_t* post_tf, int64_t* post_first,
                                 int32_t* doc_len) {
  clear_error();
  IndexRead reading(ix);
  NP_TRY(check_readable("np_hip_index_get_text_layout", ix));
  DeviceGuard g(ix->device);
  if (!g.ok) {
    set_error("hipSetDevice(%d) failed", ix->device);
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  const DeviceText& t = ix->text;
  const size_t P = (size_t)t.n_post;
  if (post_off) NP_HIP(hipMemcpy(post_off, t.post_off.get(), (size_t)(t.n_terms + 1) * 8, hipMemcpyDeviceToHost));
  if (post_doc && P > 0) NP_HIP(hipMemcpy(post_doc, t.post_doc.get(), P * 4, hipMemcpyDeviceToHost));
  if (post_tf && P > 0) NP_HIP(hipMemcpy(post_tf, t.post_tf.get(), P * 4, hipMemcpyDeviceToHost));
  if (post_first && P > 0) NP_HIP(hipMemcpy(post_first, t.post_first.get(), P * 8, hipMemcpyDeviceToHost));
  if (doc_len && ix->n_docs > 0) NP_HIP(hipMemcpy(doc_len, t.doc_len.get(), (size_t)ix->n_docs * 4, hipMemcpyDeviceToHost));
  return NP_OK;
}

}  // extern "C"
