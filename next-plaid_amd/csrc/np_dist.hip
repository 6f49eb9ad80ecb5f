// np_dist.hip -- document-sharded search below the C ABI: one process per GPU, RCCL all-gathers over xGMI.
//
// The reference has no multi-GPU path.  north_star: "the index shards by document across the 8 GPUs
// of one node with a final RCCL all-gather of per-shard top-k over xGMI".  A compiled host (the Rust crate, a C++
// service) gets the whole protocol from ONE call, np_hip_search_batch_sharded, with no torch in the process:
//
//   [subset only] local eligible-centroid bitmap -> all-gather (K/8 bytes per rank) -> OR      search.rs:350-364
//   phase A   S1-S5 on the local shard -> the shard's n_sel best rank keys                      search.rs:460-469
//   gather 1  ncclAllGather of the keys, [B][n_sel] u64 per rank
//   cut       every rank takes the global n_sel-th key per query (the reference cuts GLOBALLY)
//   phase B   exact MaxSim only for local candidates with key >= cut -> local top-k            search.rs:481-515
//   gather 2  ncclAllGather of one packed record per rank: ids | keys | scores | counts
//   merge     top-k by (exact score desc, approx rank) == the reference's final stable sort
//
// np_hip_search_batch_sharded_filtered runs the same pass on a CSR every rank evaluates from its own columns; the filters' local
// lengths ride behind the eligible bitmaps and the probe scaling reads their sums.  The keyword and hybrid calls over the shards
// are in np_text.hip, on this communicator.
//
// Every buffer is preallocated in the np_comm (grow-only), every step is enqueued on the caller's stream; the two
// payload collectives are <= 0.5 MB per rank, i.e. latency-bound on xGMI.  librccl is dlopen'ed on first use
// (librccl.so.1 resolves to the copy a host process already loaded, e.g. torch's), so the library has no link-time
// dependency on it and single-GPU users never load it.  next_plaid_amd/dist.py keeps the torch.distributed
// harness of the same protocol for the gloo CPU tests.
#include "np_internal.h"
#include "np_dist_plan.h"

#include <dlfcn.h>
#include <string.h>

#include <algorithm>
#include <mutex>

namespace np {

// ---- librccl, resolved at run time -------------------------------------------------------------------------------
struct NcclUniqueId {
  char internal[128];   // NCCL_UNIQUE_ID_BYTES
};
typedef void* NcclComm;
enum { kNcclSuccess = 0, kNcclUint8 = 1 };

struct NcclApi {
  void* lib = nullptr;
  int (*GetUniqueId)(NcclUniqueId*) = nullptr;
  int (*CommInitRank)(NcclComm*, int, NcclUniqueId, int) = nullptr;
  int (*CommDestroy)(NcclComm) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, NcclComm, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  int (*CommCount)(NcclComm, int*) = nullptr;   // optional
  std::string err;
};

static NcclApi* nccl_api() {
  static NcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* names[] = {getenv("NEXTPLAID_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      if (!n || !*n) continue;
      api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
      const char* e = dlerror();   // one call: dlerror() clears the message it returns
      api.err = e ? e : "dlopen failed";
    }
    if (!api.lib) return;
    api.GetUniqueId = (int (*)(NcclUniqueId*))dlsym(api.lib, "ncclGetUniqueId");
    api.CommInitRank = (int (*)(NcclComm*, int, NcclUniqueId, int))dlsym(api.lib, "ncclCommInitRank");
    api.CommDestroy = (int (*)(NcclComm))dlsym(api.lib, "ncclCommDestroy");
    api.AllGather = (int (*)(const void*, void*, size_t, int, NcclComm, hipStream_t))dlsym(api.lib, "ncclAllGather");
    api.GetErrorString = (const char* (*)(int))dlsym(api.lib, "ncclGetErrorString");
    api.CommCount = (int (*)(NcclComm, int*))dlsym(api.lib, "ncclCommCount");
    if (!api.GetUniqueId || !api.CommInitRank || !api.CommDestroy || !api.AllGather) {
      api.err = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / ncclAllGather";
      api.lib = nullptr;
    }
  });
  return &api;
}

static int nccl_check(int rc, const char* what) {
  if (rc == kNcclSuccess) return NP_OK;
  NcclApi* a = nccl_api();
  set_error("%s failed: %s", what, a->GetErrorString ? a->GetErrorString(rc) : "RCCL error");
  return NP_ERR_DEVICE_UNAVAILABLE;
}

}  // namespace np

using namespace np;

static int comm_common(const np_index* ix, int32_t rank, int32_t nranks, np_comm** out, const char* who) {
  if (!ix || !out || nranks < 1 || rank < 0 || rank >= nranks) {
    set_error("%s: invalid argument", who);
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  if (ix->opts.shard_count != nranks || ix->opts.shard_rank != rank) {
    set_error("%s: the handle holds shard %d/%d but the communicator is rank %d/%d", who, ix->opts.shard_rank,
              ix->opts.shard_count, rank, nranks);
    return NP_ERR_INVALID_ARGUMENT;
  }
  np_comm* c = new np_comm();
  c->rank = rank;
  c->nranks = nranks;
  c->device = ix->device;
  DeviceGuard g(ix->device);
  hipError_t e = hipHostMalloc((void**)&c->h_status, 64, hipHostMallocDefault);
  if (e != hipSuccess) {
    set_error("%s: hipHostMalloc failed: %s", who, hipGetErrorString(e));
    delete c;
    return NP_ERR_OUT_OF_MEMORY;
  }
  *c->h_status = 0;
  *out = c;
  return NP_OK;
}

extern "C" {

int np_hip_comm_unique_id(void* id128) {
  clear_error();
  if (!id128) {
    set_error("comm_unique_id: NULL argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NcclApi* a = nccl_api();
  if (!a->lib) {
    set_error("librccl is not available: %s", a->err.c_str());
    return NP_ERR_DEVICE_UNAVAILABLE;
  }
  NcclUniqueId id;
  NP_TRY(nccl_check(a->GetUniqueId(&id), "ncclGetUniqueId"));
  memcpy(id128, id.internal, 128);
  return NP_OK;
}

int np_hip_comm_create(const np_index* ix, const void* id128, int32_t rank, int32_t nranks, np_comm** out) {
  clear_error();
  if (!out) {
    set_error("comm_create: NULL out pointer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  if (nranks > 1 && !id128) {
    set_error("comm_create: invalid argument (more than one rank needs the RCCL id)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  np_comm* c = nullptr;
  NP_TRY(comm_common(ix, rank, nranks, &c, "comm_create"));
  if (id128) {   // nranks == 1 with an id still builds a real (single-rank) RCCL communicator
    NcclApi* a = nccl_api();
    if (!a->lib) {
      set_error("librccl is not available: %s", a->err.c_str());
      np_hip_comm_destroy(c);
      return NP_ERR_DEVICE_UNAVAILABLE;
    }
    DeviceGuard g(ix->device);
    NcclUniqueId id;
    memcpy(id.internal, id128, 128);
    NcclComm nc = nullptr;
    int rc = nccl_check(a->CommInitRank(&nc, nranks, id, rank), "ncclCommInitRank");
    c->comm = nc;
    if (rc != NP_OK) {
      c->comm = nullptr;
      np_hip_comm_destroy(c);
      return rc;
    }
  }
  *out = c;
  return NP_OK;
}

int np_hip_comm_create_hosted(const np_index* ix, int32_t rank, int32_t nranks, np_all_gather_host_fn all_gather,
                              void* ctx, int32_t flags, np_comm** out) {
  clear_error();
  if (!out) {
    set_error("comm_create_hosted: NULL out pointer");
    return NP_ERR_INVALID_ARGUMENT;
  }
  *out = nullptr;
  if (!all_gather) {
    set_error("comm_create_hosted: NULL all-gather callback");
    return NP_ERR_INVALID_ARGUMENT;
  }
  np_comm* c = nullptr;
  NP_TRY(comm_common(ix, rank, nranks, &c, "comm_create_hosted"));
  c->host_fn = all_gather;
  c->host_ctx = ctx;
  c->host_flags = flags;
  *out = c;
  return NP_OK;
}

void np_hip_comm_destroy(np_comm* c) {
  if (!c) return;
  {
    DeviceGuard g(c->device);
    if (c->comm) (void)nccl_api()->CommDestroy((NcclComm)c->comm);
    DevBuf* all[] = {&c->keys_local, &c->keys_all,    &c->cut,          &c->pack_local, &c->pack_all, &c->elig_local,
                     &c->elig_all,   &c->elig_global, &c->filt,         &c->filt_csr,   &c->glen,     &c->tx_cnt_local,
                     &c->tx_cnt_all, &c->tx_local,    &c->tx_all,       &c->tx_src,     &c->lists};
    for (DevBuf* b : all) b->release();
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_small) (void)hipHostFree(c->h_small);
    if (c->h_status) (void)hipHostFree(c->h_status);
  }
  delete c;
}

int np_hip_comm_status(np_comm* c, int32_t* failed_rank, int32_t* code) {
  if (!c || !c->h_status) return NP_ERR_INVALID_ARGUMENT;
  const uint64_t w = __atomic_exchange_n(c->h_status, 0ull, __ATOMIC_ACQ_REL);
  if (failed_rank) *failed_rank = w ? (int32_t)(w >> 32) - 1 : -1;
  if (code) *code = (int32_t)(w & 0xffffffffu);
  return NP_OK;
}

int np_hip_comm_info(np_comm* c, int32_t* transport, int32_t* nranks, int32_t* rccl_ranks) {
  if (!c) return NP_ERR_INVALID_ARGUMENT;
  if (transport) *transport = c->host_fn ? NP_COMM_HOSTED : (c->comm ? NP_COMM_RCCL : NP_COMM_LOCAL);
  if (nranks) *nranks = c->nranks;
  if (rccl_ranks) {
    int n = 0;
    NcclApi* a = c->comm ? nccl_api() : nullptr;
    if (a && a->CommCount && a->CommCount((NcclComm)c->comm, &n) != kNcclSuccess) n = 0;
    *rccl_ranks = n;
  }
  return NP_OK;
}

}  // extern "C"

// send -> recv[nranks][bytes].  RCCL: ncclAllGather on the caller's stream.  Hosted: the bytes go through pinned host
// staging and the host's own transport (the stream is synchronised: the callback is host code).  A communicator with
// neither is the one-rank case (a device copy).  *h_recv (hosted only) = the gathered bytes in host memory.
int np::comm_all_gather(np_comm* c, const void* send, void* recv, size_t bytes, hipStream_t st, const char** h_recv) {
  if (h_recv) *h_recv = nullptr;
  if (c->host_fn) {
    const size_t need = bytes * ((size_t)c->nranks + 1);
    if (need > c->h_stage_cap) {
      if (c->h_stage) (void)hipHostFree(c->h_stage);
      c->h_stage = nullptr;
      c->h_stage_cap = 0;
      NP_HIP(hipHostMalloc((void**)&c->h_stage, need + 4096, hipHostMallocDefault));
      c->h_stage_cap = need + 4096;
    }
    NP_HIP(hipMemcpyAsync(c->h_stage, send, bytes, hipMemcpyDeviceToHost, st));
    NP_HIP(hipStreamSynchronize(st));
    const int rc = c->host_fn(c->host_ctx, c->h_stage, c->h_stage + bytes, (int64_t)bytes);
    if (rc != 0) {
      set_error("hosted all-gather callback failed with %d", rc);
      return NP_ERR_DEVICE_UNAVAILABLE;
    }
    NP_HIP(hipMemcpyAsync(recv, c->h_stage + bytes, bytes * (size_t)c->nranks, hipMemcpyHostToDevice, st));
    if (h_recv) *h_recv = c->h_stage + bytes;
    return NP_OK;
  }
  if (!c->comm) {
    NP_HIP(hipMemcpyAsync(recv, send, bytes, hipMemcpyDeviceToDevice, st));
    return NP_OK;
  }
  return nccl_check(nccl_api()->AllGather(send, recv, bytes, kNcclUint8, (NcclComm)c->comm, st), "ncclAllGather");
}

int np::comm_small_pin(np_comm* c, size_t bytes, char** out) {
  if (bytes > c->h_small_cap) {
    if (c->h_small) (void)hipHostFree(c->h_small);
    c->h_small = nullptr;
    c->h_small_cap = 0;
    NP_HIP(hipHostMalloc((void**)&c->h_small, bytes + 4096, hipHostMallocDefault));
    c->h_small_cap = bytes + 4096;
  }
  *out = c->h_small;
  return NP_OK;
}

static uint64_t status_word(int rank, int rc) { return dist_status_word(rank, rc); }
static uint64_t gathered_failure(const char* h_all, size_t rec, size_t off_status, int G) {
  return dist_first_failure(h_all, rec, off_status, G);
}

// glen[s] = the sum over the ranks of the local lengths that ride behind the eligible bitmaps of a filtered call's record
__global__ void sum_lens_kernel(const char* __restrict__ all, int64_t rec_bytes, int64_t off, int G, int64_t n,
                                int64_t* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  int64_t v = 0;
  for (int g = 0; g < G; ++g) v += ((const int64_t*)(all + (int64_t)g * rec_bytes + off))[s];
  out[s] = v;
}

// the arguments of a sharded semantic pass that every rank sees alike, before any lock or collective
static int check_sharded_call(const np_index* ix, np_comm* c, int32_t B, const np_search_params* params, const int64_t* d_out_ids,
                              const float* d_out_scores, const int32_t* d_out_counts, void* stream) {
  if (!ix || !c || !params || !stream) {
    set_error("search_batch_sharded: NULL index / communicator / params / stream (the collectives need the caller's stream)");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (B < 0 || (B > 0 && (!d_out_counts || (params->top_k > 0 && (!d_out_ids || !d_out_scores))))) {
    set_error("search_batch_sharded: invalid argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

int np::search_batch_sharded_locked(const np_index* ix, np_comm* c, const float* d_queries, const int32_t* d_q_tok_offsets,
                                    const int32_t* h_q_tok_offsets, int32_t B, int32_t dim, const np_search_params* params,
                                    const ShardSubsets& ss, int64_t* d_out_ids, float* d_out_scores, int32_t* d_out_counts,
                                    void* stream, int rc0, const char* rc0_msg) {
  NP_TRY(check_sharded_call(ix, c, B, params, d_out_ids, d_out_scores, d_out_counts, stream));
  if (B == 0) return NP_OK;
  DeviceGuard g(ix->device);
  hipStream_t st = (hipStream_t)stream;
  const int G = c->nranks;
  const int n_sel = np_hip_n_sel(params), ns1 = std::max(n_sel, 1), k = params->top_k, k1 = std::max(k, 1);
  // Failures every rank sees alike (they depend on the arguments only) return before the first collective.
  if (!select_cut_fits(G, n_sel)) {
    set_error("Search failed: %d shards x %d re-rank candidates exceed the 16384-key window of the global cut", G, n_sel);
    return NP_ERR_SEARCH;
  }

  // The protocol never leaves a peer blocked in a collective: every exchange record ends in a status word
  // (0, or np_status | (rank + 1) << 32).  A rank whose LOCAL work fails (out of memory for its workspace, a batch that
  // does not fit its slice, a launch error) still takes part in both all-gathers with empty data and its status; the
  // cut kernel then lets nothing survive, the merge empties every query and leaves the word in pinned host memory
  // (np_hip_comm_status, valid once the stream is synchronised); the failing rank returns its own error at once.  With
  // the hosted transport the gathered bytes pass through the host anyway, so every rank reads the statuses after
  // gather 1 and returns NP_ERR_SEARCH there (flag NP_COMM_DEFERRED_STATUS keeps the device-side propagation).
  // What stays fatal is a failure to reserve the communicator's own few-hundred-KB buffers, before the first collective.
  const bool batched = params->centroid_batch_size > 0 && ix->K > params->centroid_batch_size;
  const int64_t S = ss.rows();
  const bool need_elig = S > 0 && !batched;
  const size_t o_keys = (size_t)B * k1 * 8, o_sc = o_keys * 2, o_cnt = o_sc + (size_t)B * k1 * 4;
  const size_t o_st2 = (o_cnt + (size_t)B * 4 + 15) / 16 * 16, rec2 = o_st2 + 16;
  const size_t o_st1 = (size_t)B * ns1 * 8, rec1 = o_st1 + 16;
  const int64_t words = np_hip_elig_words(ix);
  // a filtered call's CSR holds this shard's part of every subset: the local lengths ride behind the bitmaps (K is padded to
  // 64: the bitmaps end on an 8-byte boundary) and the probe scaling reads their sums.  The batched probe scales nothing.
  const bool lens = need_elig && ss.h_local_lens != nullptr;
  const DistEligRec er = dist_elig_record(S, words, lens);
  const size_t b_elig = er.o_lens, rec0 = er.bytes;
  {
    if (need_elig) {
      NP_TRY(c->elig_local.reserve(rec0));
      NP_TRY(c->elig_all.reserve((size_t)G * rec0));
      NP_TRY(c->elig_global.reserve(rec0));
    }
    if (lens) NP_TRY(c->glen.reserve((size_t)S * 8));
    NP_TRY(c->keys_local.reserve(rec1));
    NP_TRY(c->keys_all.reserve((size_t)G * rec1));
    NP_TRY(c->cut.reserve((size_t)B * 8));
    NP_TRY(c->pack_local.reserve(rec2));
    NP_TRY(c->pack_all.reserve((size_t)G * rec2));
  }
  const bool host_check = c->host_check();
  int rc = rc0;            // this rank's first local failure
  std::string rc_msg = rc0 != NP_OK && rc0_msg ? rc0_msg : "";   // ... and its message (later calls overwrite the thread-local one)
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

  // ---- eligible centroids of the subset, OR-ed over the shards (dense path only: search.rs:350-364 vs :542-545)
  const uint32_t* elig = nullptr;
  const int64_t* glen = nullptr;
  if (need_elig) {
    if (rc != NP_OK ||
        !local(ss.h_off ? np_hip_subsets_eligible(ix, ss.d_ids, ss.d_off, ss.h_off, ss.n, c->elig_local.as<uint32_t>(), st)
                        : np_hip_subset_eligible(ix, ss.d_ids, ss.len, c->elig_local.as<uint32_t>(), st)))
      (void)hipMemsetAsync(c->elig_local.p, 0, b_elig, st);
    if (lens) {   // (the pinned area is free: the filters' evaluation synchronised the stream after its previous use)
      char* pin = nullptr;
      NP_TRY(comm_small_pin(c, (size_t)S * 8, &pin));
      if (rc == NP_OK) memcpy(pin, ss.h_local_lens, (size_t)S * 8); else memset(pin, 0, (size_t)S * 8);
      NP_HIP(hipMemcpyAsync(c->elig_local.as<char>() + b_elig, pin, (size_t)S * 8, hipMemcpyHostToDevice, st));
    }
    NP_TRY(comm_all_gather(c, c->elig_local.p, c->elig_all.p, rec0, st));
    // (the OR runs over the whole record: what it leaves behind the bitmaps is not read)
    local(np_hip_or_bitmaps(ix, c->elig_all.as<uint32_t>(), G, (int64_t)(rec0 / 4), c->elig_global.as<uint32_t>(), st));
    elig = c->elig_global.as<uint32_t>();
    if (lens) {
      sum_lens_kernel<<<(unsigned)((S + 255) / 256), 256, 0, st>>>(c->elig_all.as<char>(), (int64_t)rec0, (int64_t)b_elig, G, S,
                                                                  c->glen.as<int64_t>());
      NP_HIP(hipGetLastError());
      glen = c->glen.as<int64_t>();
    }
  }

  // ---- phase A + gather 1 + cut
  void* state = nullptr;
  if (rc == NP_OK)
    local(ss.h_off ? search_phase_a_subsets_lens(ix, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, ss.d_ids,
                                                 ss.d_off, ss.h_off, ss.n, ss.d_qsub, glen, elig,
                                                 c->keys_local.as<uint64_t>(), st, &state)
                   : np_hip_search_phase_a(ix, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, ss.d_ids, ss.len,
                                           elig, c->keys_local.as<uint64_t>(), st, &state));
  struct End {
    const np_index* ix;
    void*& s;
    ~End() {
      if (s) np_hip_search_end(ix, s);
    }
  } end{ix, state};
  char* kl = c->keys_local.as<char>();
  if (rc != NP_OK) NP_HIP(hipMemsetAsync(kl, 0, o_st1, st));   // no keys from this rank
  NP_TRY(set_status_word(ix, (uint64_t*)(kl + o_st1), status_word(c->rank, rc), st));
  const char* h_all = nullptr;
  NP_TRY(comm_all_gather(c, kl, c->keys_all.p, rec1, st, &h_all));
  if (host_check && h_all) {
    const uint64_t w = gathered_failure(h_all, rec1, o_st1, G);
    if (w) {   // every rank reads the same bytes: all leave here, none enters gather 2
      if (rc != NP_OK) return finish(rc);
      set_error("Search failed: shard %d failed with status %d; the batch was abandoned on every rank",
                (int)(w >> 32) - 1, (int)(w & 0xffffffffu));
      return NP_ERR_SEARCH;
    }
  }
  if (n_sel > 0)
    local(select_cut_strided(ix, c->keys_all.as<uint64_t>(), (int64_t)(rec1 / 8), (int64_t)(o_st1 / 8), G, B, n_sel,
                             c->cut.as<uint64_t>(), st));

  // ---- phase B into one packed record: ids [B*k] i64 | keys [B*k] u64 | scores [B*k] f32 | counts [B] i32 | status
  char* pl = c->pack_local.as<char>();
  if (rc == NP_OK && state)
    local(np_hip_search_phase_b(ix, state, n_sel > 0 ? c->cut.as<uint64_t>() : nullptr, (int64_t*)pl, (float*)(pl + o_sc),
                                (uint64_t*)(pl + o_keys), (int32_t*)(pl + o_cnt), st));
  if (rc != NP_OK) NP_HIP(hipMemsetAsync(pl, 0, o_st2, st));   // counts 0
  NP_TRY(set_status_word(ix, (uint64_t*)(pl + o_st2), status_word(c->rank, rc), st));
  // ---- gather 2 + merge
  NP_TRY(comm_all_gather(c, pl, c->pack_all.p, rec2, st, &h_all));
  NP_TRY(merge_packed_status(ix, c->pack_all.p, (int64_t)rec2, (int64_t)o_keys, (int64_t)o_sc, (int64_t)o_cnt,
                             (int64_t)o_st2,
                             /* a rank that reports the failure by its return code (its own, or -- hosted transport with the
                                host-side check -- a peer's, below) must not ALSO leave the word behind for the next healthy
                                batch's np_hip_comm_status */
                             (rc == NP_OK && !host_check) ? c->h_status : nullptr, G, B, k,
                             d_out_ids, d_out_scores, d_out_counts, st));
  if (rc != NP_OK) return finish(rc);
  if (host_check && h_all) {
    const uint64_t w = gathered_failure(h_all, rec2, o_st2, G);
    if (w) {
      set_error("Search failed: shard %d failed with status %d; the batch was abandoned on every rank",
                (int)(w >> 32) - 1, (int)(w & 0xffffffffu));
      return NP_ERR_SEARCH;
    }
  }
  return NP_OK;
}

extern "C" int np_hip_search_batch_sharded(const np_index* ix, np_comm* c, const float* d_queries,
                                           const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                           int32_t dim, const np_search_params* params, const int64_t* d_subset,
                                           int64_t subset_len, int64_t* d_out_ids, float* d_out_scores,
                                           int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(check_sharded_call(ix, c, B, params, d_out_ids, d_out_scores, d_out_counts, stream));
  std::lock_guard<std::mutex> lk(c->mu);
  return search_batch_sharded_locked(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params,
                                     ShardSubsets::single(d_subset, subset_len), d_out_ids, d_out_scores, d_out_counts, stream);
}

// Arguments every rank sees alike are checked before the first collective; `query_subset` lives on the device and is not.
extern "C" int np_hip_search_batch_sharded_subsets(const np_index* ix, np_comm* c, const float* d_queries,
                                                   const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets,
                                                   int32_t B, int32_t dim, const np_search_params* params,
                                                   const int64_t* d_subset_ids, const int64_t* d_subset_offsets,
                                                   const int64_t* h_subset_offsets, int64_t n_subsets,
                                                   const int32_t* d_query_subset, int64_t* d_out_ids, float* d_out_scores,
                                                   int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(check_device_subsets(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset, B));
  const ShardSubsets ss =
      ShardSubsets::csr(CallSubsets::device(d_subset_ids, d_subset_offsets, h_subset_offsets, n_subsets, d_query_subset));
  NP_TRY(check_sharded_call(ix, c, B, params, d_out_ids, d_out_scores, d_out_counts, stream));
  std::lock_guard<std::mutex> lk(c->mu);
  return search_batch_sharded_locked(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, ss, d_out_ids,
                                     d_out_scores, d_out_counts, stream);
}

int np::check_sharded_filters(const char* who, const np_filter* filters, int32_t n_filters, const int32_t* query_filter, int B) {
  if (n_filters < 0 || (n_filters > 0 && (!filters || (B > 0 && !query_filter)))) {
    set_error("%s: negative n_filters, or filters without programs or a query map", who);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

void np::ShardFilterScope::eval(const np_index* ix, np_comm* c, hipStream_t st, const np_filter* filters, int32_t n_filters,
                                const int32_t* query_filter, int B) {
  n = n_filters;
  any = any_scoped(query_filter, n_filters, B);
  if (!any) return;
  rc0 = filter_check_call(ix, filters, n_filters, query_filter, B, 2);
  if (rc0 == NP_OK) rc0 = filter_eval_resident(ix, st, c->filt, c->filt_csr, filters, n_filters, query_filter, B, &csr);
  zero.assign((size_t)n + 1, 0);
  lens.assign((size_t)n, 0);
  if (rc0 != NP_OK) {
    msg0 = np_hip_last_error();
    return;
  }
  for (int32_t f = 0; f < n; ++f) lens[(size_t)f] = csr.h_off[(size_t)f + 1] - csr.h_off[(size_t)f];
  sub = CallSubsets::device(csr.d_ids, csr.d_off, csr.h_off.data(), n, csr.d_qsub, query_filter);
}

np::ShardSubsets np::ShardFilterScope::shard() const {
  if (!any) return ShardSubsets::none();
  CallSubsets s = sub;
  if (rc0 != NP_OK) {   // the rank still exchanges one (empty) row per filter
    s.n = n;
    s.h_off = zero.data();
  }
  return ShardSubsets::csr(s).with_local_lens(lens.data());
}

// The filters are evaluated over the shard's own columns; what crosses the ranks beyond np_hip_search_batch_sharded_subsets'
// exchanges is every filter's local length, behind the eligible bitmaps.  A rank whose filters fail (no columns on its handle, a
// program its schema refuses) takes part with empty data like any other local failure.
extern "C" int np_hip_search_batch_sharded_filtered(const np_index* ix, np_comm* c, const float* d_queries,
                                                    const int32_t* d_q_tok_offsets, const int32_t* h_q_tok_offsets, int32_t B,
                                                    int32_t dim, const np_search_params* params, const np_filter* filters,
                                                    int32_t n_filters, const int32_t* query_filter, int64_t* d_out_ids,
                                                    float* d_out_scores, int32_t* d_out_counts, void* stream) {
  clear_error();
  NP_TRY(check_sharded_call(ix, c, B, params, d_out_ids, d_out_scores, d_out_counts, stream));
  NP_TRY(check_sharded_filters("search_batch_sharded_filtered", filters, n_filters, query_filter, B));
  if (B == 0) return NP_OK;
  std::lock_guard<std::mutex> lk(c->mu);
  DeviceGuard g(ix->device);
  ShardFilterScope scope;   // (as unsharded: a batch none of whose queries has a filter is a batch without subsets)
  scope.eval(ix, c, (hipStream_t)stream, filters, n_filters, query_filter, B);
  return search_batch_sharded_locked(ix, c, d_queries, d_q_tok_offsets, h_q_tok_offsets, B, dim, params, scope.shard(), d_out_ids,
                                     d_out_scores, d_out_counts, stream, scope.rc0, scope.msg0.c_str());
}
