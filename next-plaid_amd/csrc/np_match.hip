// np_match.hip -- text predicates on the device: the dictionary text of a CODE column in HBM (np_hip_index_set_column_text),
// np_hip_text_match, and the match passes behind the NP_F_MATCH leaves of a filter (np_filter.hip).
//
// The work is one table lookup per byte per string.  match_kernel<TAB_LDS>: a block owns 256 consecutive strings of the
// dictionary, which are one contiguous run of the byte array.  It stages that run tile by tile (NP_MATCH_TILE_BYTES, 16-byte
// loads from a 16-byte aligned base) into LDS and every lane walks its own string out of the tile, its state carried in a
// register from tile to tile: a string that straddles or exceeds a tile needs nothing special.  class_of[256] is in LDS always;
// the table is copied there too when it fits the plan's budget (TAB_LDS) and read from global memory through the caches when
// not.  Table entries carry the target state's flags (np_match_plan.h), so a lane that reaches MATCHED or DEAD stops without a
// second lookup, and the block stops staging once every lane has its verdict: a very long string keeps its own block (whose
// other 255 verdicts are decided by then) and no other, and np_hip_index_set_column_text refuses a string of more than
// NP_MATCH_MAX_STRING_BYTES, which bounds that block's time.  Known cost of this mapping: with strings much longer than
// tile / 256 bytes only a few of a block's lanes have bytes in the staged tile and the others wait at the barrier.  A wave's
// 64 verdicts leave as one ballot, two u32 words; no atomics, so the bits do not depend on the chunking or on the run.
#include "np_internal.h"
#include "np_match_plan.h"
#include <chrono>
#include <string.h>

namespace np {

constexpr int MATCH_TPB = (int)NP_MATCH_BLOCK_STRINGS;

struct MatchDfaDev {
  const uint8_t* image;   // class_of[256] | u16 table, 256-byte aligned
  int32_t n_classes;
  uint32_t start;         // the start state's entry
  int32_t image_bytes;    // multiple of 16
  int32_t out_row;        // row of the launch's bits this DFA writes
};

struct MatchP {
  const uint8_t* bytes;
  const int64_t* off;
  int64_t s0, ns;             // the chunk's strings [s0, s0 + ns), s0 a multiple of 256
  const MatchDfaDev* dfas;    // of the launch: blockIdx.y
  uint32_t* bits;             // [rows][row_words], bit of string s at (s - s0)
  int64_t row_words;
  int32_t tile;
};

template <bool TAB_LDS>
__global__ void __launch_bounds__(MATCH_TPB) match_kernel(MatchP p) {
  extern __shared__ uint4 match_smem[];
  uint8_t* tile = reinterpret_cast<uint8_t*>(match_smem);
  uint8_t* cls = tile + p.tile;
  const MatchDfaDev D = p.dfas[blockIdx.y];
  {
    const int n16 = TAB_LDS ? D.image_bytes / 16 : 16;
    const uint4* src = reinterpret_cast<const uint4*>(D.image);
    uint4* dst = reinterpret_cast<uint4*>(cls);
    for (int i = threadIdx.x; i < n16; i += MATCH_TPB) dst[i] = src[i];
  }
  const uint16_t* tab = TAB_LDS ? reinterpret_cast<const uint16_t*>(cls + 256) : reinterpret_cast<const uint16_t*>(D.image + 256);
  const int nc = D.n_classes;
  const int64_t first = p.s0 + (int64_t)blockIdx.x * MATCH_TPB, end = p.s0 + p.ns;
  const int64_t last = first + MATCH_TPB < end ? first + MATCH_TPB : end;
  const int64_t s = first + threadIdx.x;
  const bool live = s < last;
  const int64_t B1 = p.off[last];
  const int64_t b = live ? p.off[s] : B1, e = live ? p.off[s + 1] : B1;
  uint32_t cur = D.start;
  int64_t pos = b;
  bool done = !live || pos >= e || (cur & (NP_MATCH_E_MATCHED | NP_MATCH_E_DEAD));
  for (int64_t t0 = p.off[first] & ~(int64_t)15; t0 < B1; t0 += p.tile) {
    // also the barrier between the walk of the previous tile (or the table copy) and the stores of this one
    if (!__syncthreads_or(!done)) break;
    const int64_t left = ((B1 + 15) & ~(int64_t)15) - t0;   // the byte array is padded to a multiple of 16
    const int n = left < p.tile ? (int)left : p.tile;
    for (int i = threadIdx.x * 16; i < n; i += MATCH_TPB * 16)
      *reinterpret_cast<uint4*>(tile + i) = *reinterpret_cast<const uint4*>(p.bytes + t0 + i);
    __syncthreads();
    if (!done && pos < t0 + n) {
      const int64_t tend = e < t0 + n ? e : t0 + n;
      int i = (int)(pos - t0);
      const int iend = (int)(tend - t0);
      while (i < iend) {
        cur = tab[(cur & NP_MATCH_E_STATE) * nc + cls[tile[i]]];
        ++i;
        if (cur & (NP_MATCH_E_MATCHED | NP_MATCH_E_DEAD)) break;
      }
      pos = t0 + i;
      done = pos >= e || (cur & (NP_MATCH_E_MATCHED | NP_MATCH_E_DEAD));
    }
  }
  const bool hit = live && ((cur & NP_MATCH_E_MATCHED) || (pos >= e && (cur & NP_MATCH_E_ACCEPT)));
  const unsigned long long word = __ballot(hit);
  if ((threadIdx.x & 63) == 0) {
    uint32_t* out = p.bits + (int64_t)D.out_row * p.row_words + ((int64_t)blockIdx.x * MATCH_TPB + threadIdx.x) / 32;
    out[0] = (uint32_t)word;
    out[1] = (uint32_t)(word >> 32);
  }
}


// One launch group: DFAs [0, n) described by host-built images, over strings [s0, s0 + ns) of a column, verdicts to
// d_bits[row][row_words].  d_work receives the images and the descriptor table (the caller sized it: sum of up256(image) + 4096).
struct MatchImage {
  std::vector<uint8_t> bytes;
  MatchDfaInfo info;
  uint32_t start = 0;
  bool lds = false;
};
static int match_launch(const DeviceColumn& col, hipStream_t st, const std::vector<MatchImage>& imgs, int32_t i0, int32_t n,
                        int64_t s0, int64_t ns, uint32_t* d_bits, int64_t row_words, char* d_work, int32_t tile) {
  if (ns <= 0 || n <= 0) return NP_OK;
  std::vector<MatchDfaDev> h_lds, h_glb;
  char* at = d_work;
  int32_t lds_bytes = 0;
  for (int32_t i = 0; i < n; ++i) {
    const MatchImage& im = imgs[i0 + i];
    NP_HIP(hipMemcpyAsync(at, im.bytes.data(), im.bytes.size(), hipMemcpyHostToDevice, st));
    const MatchDfaDev d{(const uint8_t*)at, im.info.n_classes, im.start, (int32_t)im.info.image_bytes, i};
    (im.lds ? h_lds : h_glb).push_back(d);
    if (im.lds) lds_bytes = std::max(lds_bytes, (int32_t)im.info.image_bytes);
    at += up256(im.bytes.size());
  }
  MatchDfaDev* d_tab = (MatchDfaDev*)at;   // [lds DFAs | global DFAs], at most 4096 bytes: a group holds at most MATCH_GROUP_MAX = 170 DFAs
  std::vector<MatchDfaDev> h_tab(h_lds);
  h_tab.insert(h_tab.end(), h_glb.begin(), h_glb.end());
  NP_HIP(hipMemcpyAsync(d_tab, h_tab.data(), h_tab.size() * sizeof(MatchDfaDev), hipMemcpyHostToDevice, st));
  NP_HIP(hipStreamSynchronize(st));   // pageable sources
  MatchP p{col.text.get(), col.text_off.get(), s0, ns, d_tab, d_bits, row_words, tile};
  const unsigned blocks = (unsigned)((ns + MATCH_TPB - 1) / MATCH_TPB);
  if (!h_lds.empty())
    match_kernel<true><<<dim3(blocks, (unsigned)h_lds.size()), MATCH_TPB, (size_t)tile + (size_t)lds_bytes, st>>>(p);
  if (!h_glb.empty()) {
    p.dfas = d_tab + h_lds.size();
    match_kernel<false><<<dim3(blocks, (unsigned)h_glb.size()), MATCH_TPB, (size_t)tile + 256, st>>>(p);
  }
  NP_HIP(hipGetLastError());
  return NP_OK;
}
constexpr int32_t MATCH_GROUP_MAX = 4096 / (int32_t)sizeof(MatchDfaDev);

template <class W>
static int match_make_image(const W* words, int64_t n_words, int32_t dfa, int32_t lds_budget, bool checked, MatchImage* out) {
  char why[200];
  if (checked) {
    out->info = match_checked_info(words);
  } else if (match_check_dfa(words, n_words, dfa, why, sizeof why, &out->info) != 0) {
    set_error("Text match failed: %s", why);
    return NP_ERR_INVALID_ARGUMENT;
  }
  out->bytes.resize((size_t)out->info.image_bytes);
  out->start = match_build_image(words, out->info, out->bytes.data());
  out->lds = out->info.image_bytes - 256 <= lds_budget;
  return NP_OK;
}

static int match_check_column(const DeviceIndex* ix, int32_t column, const char* who) {
  if (column < 0 || column >= (int32_t)ix->columns.size()) {
    set_error("%s: column %d is not one of the handle's %d columns", who, column, (int)ix->columns.size());
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (ix->columns[column].type != NP_COL_CODE) {
    set_error("%s: column %d is not a CODE column", who, column);
    return NP_ERR_INVALID_ARGUMENT;
  }
  return NP_OK;
}

int match_check_text(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters) {
  for (int32_t f = 0; f < n_filters; ++f)
    for (int i = 0; i < filters[f].n_ops; ++i) {
      const np_filter_op& o = filters[f].ops[i];
      if (o.op == NP_F_MATCH && ix->columns[o.column].n_strings == 0) {   // the column index was checked with the program
        set_error("Filter failed: filter %d, op %d: column %d has no text on the device (np_hip_index_set_column_text)", f, i,
                  o.column);
        return NP_ERR_INVALID_ARGUMENT;
      }
    }
  return NP_OK;
}

int match_collect(const DeviceIndex* ix, const np_filter* filters, int32_t n_filters, std::vector<MatchJob>* jobs,
                  std::vector<int64_t>* op_bit_word0, int64_t* bit_words, int64_t* work_bytes) {
  jobs->clear();
  op_bit_word0->clear();
  *bit_words = 0;
  *work_bytes = 0;
  for (int32_t f = 0; f < n_filters; ++f)
    for (int i = 0; i < filters[f].n_ops; ++i) {
      const np_filter_op& o = filters[f].ops[i];
      if (o.op != NP_F_MATCH) continue;
      const DeviceColumn& col = ix->columns[o.column];
      const int64_t* w = filters[f].values + o.first_value;   // the range was checked with the program
      int64_t j = 0;
      for (; j < (int64_t)jobs->size(); ++j)
        if ((*jobs)[j].column == o.column && (*jobs)[j].n_words == o.n_values &&
            ((*jobs)[j].words == w || memcmp((*jobs)[j].words, w, (size_t)o.n_values * 8) == 0))
          break;
      if (j == (int64_t)jobs->size()) {
        const MatchDfaInfo info = match_checked_info(w);   // filter_check_program passed the table
        jobs->push_back(MatchJob{o.column, w, o.n_values, info.image_bytes, *bit_words});
        // whole blocks of verdict words: the kernel writes every word of its last block
        *bit_words += (col.n_strings + NP_MATCH_BLOCK_STRINGS - 1) / NP_MATCH_BLOCK_STRINGS * (NP_MATCH_BLOCK_STRINGS / 32);
        *work_bytes = std::max<int64_t>(*work_bytes, (int64_t)up256((size_t)info.image_bytes) + 4096);
      }
      op_bit_word0->push_back((*jobs)[j].bit_word0);
    }
  return NP_OK;
}

int match_run_jobs(const DeviceIndex* ix, hipStream_t st, const std::vector<MatchJob>& jobs, uint32_t* d_bits, char* d_work) {
  const int32_t lds_budget = ix->tune.match_lds * 1024;
  std::vector<MatchImage> img(1);
  for (size_t j = 0; j < jobs.size(); ++j) {
    const DeviceColumn& col = ix->columns[jobs[j].column];
    NP_TRY(match_make_image(jobs[j].words, jobs[j].n_words, (int32_t)j, lds_budget, true, &img[0]));
    const int64_t row_words = (col.n_strings + NP_MATCH_BLOCK_STRINGS - 1) / NP_MATCH_BLOCK_STRINGS * (NP_MATCH_BLOCK_STRINGS / 32);
    NP_TRY(match_launch(col, st, img, 0, 1, 0, col.n_strings, d_bits + jobs[j].bit_word0, row_words, d_work, NP_MATCH_TILE_BYTES));
    NP_HIP(hipStreamSynchronize(st));   // d_work is reused by the next job
  }
  return NP_OK;
}

}  // namespace np

using namespace np;

extern "C" {

int np_hip_index_set_column_text(np_index* ix, int32_t column, const uint8_t* bytes, const int64_t* offsets, int64_t n_strings) {
  clear_error();
  if (!ix) {
    set_error("set_column_text: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(match_check_column(ix, column, "set_column_text"));
  DeviceColumn& col = ix->columns[column];
  if (n_strings < 0) {
    set_error("set_column_text: negative n_strings");
    return NP_ERR_INVALID_ARGUMENT;
  }
  DeviceGuard g(ix->device);
  if (n_strings == 0) {
    col.text.reset();
    col.text_off.reset();
    ix->device_bytes -= col.text_acct;
    ix->coltext_bytes -= col.text_acct;
    col.text_acct = 0;
    col.n_strings = col.n_text_bytes = 0;
    return NP_OK;
  }
  if (!offsets) {
    set_error("set_column_text: NULL offsets");
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (col.min_code < 0 || n_strings <= col.max_code) {
    set_error("set_column_text: column %d holds codes %d..%d, which %lld strings do not cover", column, col.min_code, col.max_code,
              (long long)n_strings);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (offsets[0] != 0) {
    set_error("set_column_text: offsets[0] is %lld, not 0", (long long)offsets[0]);
    return NP_ERR_INVALID_ARGUMENT;
  }
  for (int64_t s = 0; s < n_strings; ++s)
    if (offsets[s + 1] < offsets[s]) {
      set_error("set_column_text: offsets[%lld] = %lld is below offsets[%lld] = %lld", (long long)s + 1, (long long)offsets[s + 1],
                (long long)s, (long long)offsets[s]);
      return NP_ERR_INVALID_ARGUMENT;
    }
  for (int64_t s = 0; s < n_strings; ++s)
    if (offsets[s + 1] - offsets[s] > NP_MATCH_MAX_STRING_BYTES) {
      set_error("set_column_text: string %lld has %lld bytes, at most %lld (one lane walks one string)", (long long)s,
                (long long)(offsets[s + 1] - offsets[s]), (long long)NP_MATCH_MAX_STRING_BYTES);
      return NP_ERR_INVALID_ARGUMENT;
    }
  const int64_t n_bytes = offsets[n_strings];
  if (n_bytes > 0 && !bytes) {
    set_error("set_column_text: NULL bytes");
    return NP_ERR_INVALID_ARGUMENT;
  }
  // built beside the old text and swapped in whole: a failed allocation leaves the previous text in place
  DevPtr<uint8_t> d_text;
  DevPtr<int64_t> d_off;
  size_t acct = 0;
  const size_t padded = ((size_t)n_bytes + 15) / 16 * 16 + 16;
  NP_TRY(d_text.alloc(padded, &acct));
  NP_TRY(d_off.alloc((size_t)n_strings + 1, &acct));
  NP_HIP(hipMemset(d_text.get(), 0, padded));
  if (n_bytes > 0) NP_HIP(hipMemcpy(d_text.get(), bytes, (size_t)n_bytes, hipMemcpyHostToDevice));
  NP_HIP(hipMemcpy(d_off.get(), offsets, ((size_t)n_strings + 1) * 8, hipMemcpyHostToDevice));
  col.text = std::move(d_text);
  col.text_off = std::move(d_off);
  ix->device_bytes = ix->device_bytes - col.text_acct + acct;
  ix->coltext_bytes = ix->coltext_bytes - col.text_acct + acct;
  col.text_acct = acct;
  col.n_strings = n_strings;
  col.n_text_bytes = n_bytes;
  return NP_OK;
}

int np_hip_text_match(const np_index* ix, int32_t column, const np_dfa* dfas, int32_t n_dfas, uint32_t* out_bits,
                      np_match_report* report) {
  clear_error();
  IndexRead reading(ix);   // an append waits for this call and holds later ones back (np_internal.h)
  const auto t_begin = std::chrono::steady_clock::now();
  if (report) memset(report, 0, sizeof *report);
  if (!ix) {
    set_error("Text match failed: NULL index");
    return NP_ERR_INVALID_ARGUMENT;
  }
  NP_TRY(match_check_column(ix, column, "Text match failed"));
  const DeviceColumn& col = ix->columns[column];
  if (col.n_strings == 0) {
    set_error("Text match failed: column %d has no text on the device (np_hip_index_set_column_text)", column);
    return NP_ERR_INVALID_ARGUMENT;
  }
  if (n_dfas < 0 || (n_dfas > 0 && (!dfas || !out_bits))) {
    set_error("Text match failed: %s", n_dfas < 0 ? "negative n_dfas" : !dfas ? "NULL dfas" : "NULL out_bits");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const int32_t lds_budget = ix->tune.match_lds * 1024;
  std::vector<MatchImage> img((size_t)n_dfas);
  std::vector<int64_t> sizes((size_t)n_dfas);
  for (int32_t d = 0; d < n_dfas; ++d) {
    NP_TRY(match_make_image(dfas[d].words, dfas[d].n_words, d, lds_budget, false, &img[d]));
    sizes[d] = (int64_t)up256((size_t)img[d].info.image_bytes);
  }
  MatchPlan plan;
  const int64_t budget = ix->ws_budget.load(std::memory_order_relaxed);
  if (!match_plan(budget, sizes.data(), n_dfas, col.n_strings, lds_budget, &plan)) {
    set_error("Text match failed: one DFA over %lld strings does not fit the workspace budget of %lld bytes",
              (long long)NP_MATCH_BLOCK_STRINGS, (long long)budget);
    return NP_ERR_OUT_OF_MEMORY;
  }
  plan.dfas = std::min(plan.dfas, MATCH_GROUP_MAX);
  if (report) {
    report->tile_bytes = plan.tile_bytes;
    report->table_lds_bytes = plan.table_lds_bytes;
    for (int32_t d = 0; d < n_dfas; ++d) ++(img[d].lds ? report->n_lds : report->n_global);
    report->bytes_scanned = col.n_text_bytes * n_dfas;
  }
  if (n_dfas == 0) return NP_OK;
  DeviceGuard g(ix->device);
  ContextUse use;
  NP_TRY(use.begin(ix, nullptr));
  DevBuf& scratch = use.filter_scratch();
  const size_t b_img = up256((size_t)plan.image_bytes) + 4096, b_bits = up256((size_t)plan.dfas * plan.chunk_words() * 4);
  NP_TRY(scratch.reserve(b_img + b_bits));
  char* d_work = scratch.as<char>();
  uint32_t* d_bits = (uint32_t*)(d_work + b_img);
  const int64_t out_words = (col.n_strings + 31) / 32;
  int32_t n_chunks = 0;
  for (int32_t d0 = 0; d0 < n_dfas; d0 += plan.dfas) {
    const int32_t nd = std::min(plan.dfas, n_dfas - d0);
    for (int64_t s0 = 0; s0 < col.n_strings; s0 += plan.strings) {
      const int64_t ns = std::min(plan.strings, col.n_strings - s0);
      NP_TRY(match_launch(col, use.stream, img, d0, nd, s0, ns, d_bits, plan.chunk_words(), d_work, plan.tile_bytes));
      const int64_t w0 = s0 / 32, nw = (ns + 31) / 32;
      for (int32_t d = 0; d < nd; ++d)
        NP_HIP(hipMemcpyAsync(out_bits + (int64_t)(d0 + d) * out_words + w0, d_bits + (int64_t)d * plan.chunk_words(),
                              (size_t)nw * 4, hipMemcpyDeviceToHost, use.stream));
      NP_HIP(hipStreamSynchronize(use.stream));   // the images and the bits are reused by the next chunk
      ++n_chunks;
    }
  }
  if (report) {
    report->n_chunks = n_chunks;
    report->ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return NP_OK;
}

}  // extern "C"
