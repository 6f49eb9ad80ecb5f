// np_remove_plan.h -- the host side of np_hip_index_remove that needs no device: the removed ids as the library takes them
// (in range, sorted, each once), the renumbering of a surviving id, and the schedule of launches that compacts a per-token
// array IN PLACE.  Plain C++; tests/cpp/remove_plan_check.cpp runs all of it stand-alone.
//
// The in-place move.  Surviving tokens keep their order, so token t of the old array goes to t - shift(t) with a shift that only
// grows: every destination lies at or below its source.  The hazard is inside one launch: a workgroup may write where another
// workgroup of the same launch has not read yet.  Stream order between launches is the only ordering relied on, so the moved
// range -- from the first removed token to the end -- is cut into slabs of `slab` SOURCE tokens, taken in
// ascending order, and the survivors of a slab [s0, s1) -- destination [d0, d1), their sources inside [f, l) with f the first
// and l - 1 the last surviving token of the slab -- are moved by
//   DIRECT   one launch, when d1 <= f: nothing it writes is read by it.  True as soon as the tokens removed in front of the
//            slab are at least the slab's survivors (d1 - d0 <= f - d0);
//   STAGED   a gather launch into the staging buffer (at most `slab` rows) and a copy launch out of it.
// A later slab's sources lie at or behind l >= d1, so no launch overwrites what a later one reads.  A slab without a survivor
// gives no launch.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace np {

constexpr int64_t NP_REMOVE_SLAB_DEFAULT = (int64_t)1 << 21;   // tokens per slab: a 128 MiB staging buffer at 64-byte rows

// the ids a remove acts on: those inside [0, n_docs), ascending, each once
inline std::vector<int64_t> remove_ids_in_range(const int64_t* ids, int64_t n_ids, int64_t n_docs) {
  std::vector<int64_t> v;
  for (int64_t i = 0; i < n_ids; ++i)
    if (ids[i] >= 0 && ids[i] < n_docs) v.push_back(ids[i]);
  std::sort(v.begin(), v.end());
  v.erase(std::unique(v.begin(), v.end()), v.end());
  return v;
}

// the new id of surviving document d: d minus the removed ids BELOW it (delete.rs:204-209; lower_bound, d itself is not removed)
inline int64_t remove_new_id(const std::vector<int64_t>& removed, int64_t d) {
  return d - (int64_t)(std::lower_bound(removed.begin(), removed.end(), d) - removed.begin());
}

enum RemoveMode : int32_t { NP_REMOVE_DIRECT = 0, NP_REMOVE_GATHER = 1, NP_REMOVE_COPY = 2 };

// One launch, in tokens.  DIRECT: the survivors among source tokens [src0, src1) of the array -> its tokens [dst0, dst1).
// GATHER: the same survivors -> rows [0, dst1 - dst0) of the staging buffer.  COPY: those rows -> tokens [dst0, dst1) (src0 /
// src1 repeat the gather's, for the record: the launch reads the staging buffer only).
struct RemoveLaunch {
  int32_t mode;
  int64_t src0, src1, dst0, dst1;
};

struct RemovePlan {
  std::vector<RemoveLaunch> launches;
  int64_t first_moved = 0;     // tokens in front of it are not touched
  int64_t new_tokens = 0;      // tokens of the compacted array
  int64_t staging_rows = 0;    // the most rows a gather puts into the staging buffer (<= slab)
  int64_t staging_bytes = 0;   // ... times row_bytes
  int64_t direct_tokens = 0, staged_tokens = 0;
};

// off [n_docs + 1]: the old token offsets; keep [n_docs]: 1 = the document survives; row_bytes: bytes per token of the widest
// array moved through the staging buffer; slab: source tokens per slab (< 1: the default)
inline RemovePlan remove_plan(const int64_t* off, const uint8_t* keep, int64_t n_docs, int64_t row_bytes, int64_t slab) {
  RemovePlan p;
  if (slab < 1) slab = NP_REMOVE_SLAB_DEFAULT;
  int64_t first = 0;
  while (first < n_docs && (keep[first] || off[first + 1] == off[first])) ++first;   // a removed document without tokens moves nothing
  const int64_t T = off[n_docs];
  p.first_moved = first < n_docs ? off[first] : T;
  p.new_tokens = p.first_moved;
  int64_t d = first;          // the document the walk stands in
  int64_t dst = p.first_moved;   // survivors in front of the slab = the slab's first destination
  for (int64_t s0 = p.first_moved; s0 < T; s0 += slab) {
    const int64_t s1 = std::min(T, s0 + slab);
    int64_t f = -1, l = -1, kept = 0;
    // the surviving tokens of [s0, s1): documents are cut at the slab's edges
    while (d < n_docs && off[d] < s1) {
      const int64_t a = std::max(off[d], s0), b = std::min(off[d + 1], s1);
      if (keep[d] && b > a) {
        if (f < 0) f = a;
        l = b;
        kept += b - a;
      }
      if (off[d + 1] > s1) break;   // the document goes on in the next slab
      ++d;
    }
    if (kept == 0) continue;
    const int64_t d0 = dst, d1 = dst + kept;
    dst = d1;
    if (d1 <= f) {
      p.launches.push_back(RemoveLaunch{NP_REMOVE_DIRECT, f, l, d0, d1});
      p.direct_tokens += kept;
    } else {
      p.launches.push_back(RemoveLaunch{NP_REMOVE_GATHER, f, l, d0, d1});
      p.launches.push_back(RemoveLaunch{NP_REMOVE_COPY, f, l, d0, d1});
      p.staging_rows = std::max(p.staging_rows, kept);
      p.staged_tokens += kept;
    }
  }
  p.new_tokens = dst;
  p.staging_bytes = p.staging_rows * row_bytes;
  return p;
}

}  // namespace np
