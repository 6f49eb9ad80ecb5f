// What next_plaid.hpp hands the library, and what it makes of the answer -- with the host compiler alone.
//
// The np_hip_* entries the header reaches are recording stubs in this translation unit (no library is linked; member
// functions that are not called are never emitted).  Every stub notes its name and the values behind its arguments, writes
// chosen counts and recognisable ids and scores through the output pointers and returns a chosen status.  The checks state
// the entry each call must reach and the values it must carry, how the padded rows come back (strides, query ids), and the
// policies of run_batch: NP_ERR_SEARCH under `parallel` gives empty results, anything else throws, a negative count throws.
// Built with -fsanitize=address,undefined: a row written past a buffer the header sized too small is an error here.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

constexpr int DIM = 8;
constexpr int64_t N_DOCS = 5000;
const char* MESSAGE = "Search failed: the stub said so";

struct Recorded {
  std::string entry;
  int B = -1, dim = -1, top_k = -1, precision = -1, fetch_k = -1, fusion = -1, pool_k = -1, group_size = -1, n_filters = -1;
  int sem_w = -1, kw_w = -1;
  float alpha = -1.f;
  int64_t n_sub = -2;
  np_search_params p{};
  std::vector<float> flat, sem_sc, kw_sc;
  std::vector<int32_t> off, qmap, sem_cnt, kw_cnt;
  std::vector<int64_t> sub, sid, soff, sem_ids, kw_ids, pair_docs, pair_off;
  bool sub_null = false, qmap_null = false, filters_null = false, with_scores = false, wants_matches = false;
  std::vector<std::vector<int64_t>> filter_values;
  std::vector<int32_t> filter_ops;   // the op code of every op of every filter, in order
  std::vector<std::vector<int32_t>> tq_terms, tq_off;
  std::vector<int32_t> tq_mode;
};
Recorded last;
int n_calls = 0, next_rc = NP_OK;
bool abandon = false;   // the next row call answers count -1 for query 0
int failed = 0;

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);            \
      ++failed;                                                             \
    }                                                                       \
  } while (0)

Recorded& begin(const char* entry) {
  last = Recorded{};
  last.entry = entry;
  ++n_calls;
  return last;
}

void rec_queries(const float* flat, const int32_t* off, int32_t B, int32_t dim) {
  last.B = B;
  last.dim = dim;
  last.off.assign(off, off + B + 1);
  last.flat.assign(flat, flat + (size_t)off[B] * dim);   // (an empty batch reads nothing: flat may be NULL or one float)
}
void rec_csr(const int64_t* sid, const int64_t* soff, int64_t n, const int32_t* qmap, int32_t B) {
  last.n_sub = n;
  if (soff) last.soff.assign(soff, soff + n + 1);
  if (sid && soff) last.sid.assign(sid, sid + soff[n]);
  last.qmap_null = qmap == nullptr;
  if (qmap) last.qmap.assign(qmap, qmap + B);
}
void rec_filters(const np_filter* f, int32_t n) {
  last.n_filters = n;
  last.filters_null = f == nullptr;
  for (int32_t j = 0; f && j < n; ++j) {
    for (int32_t o = 0; o < f[j].n_ops; ++o) last.filter_ops.push_back(f[j].ops[o].op);
    last.filter_values.emplace_back(f[j].values, f[j].values + f[j].n_values);
  }
}
void rec_text(const np_text_query* q, int32_t B) {
  for (int32_t i = 0; i < B; ++i) {
    last.tq_off.emplace_back(q[i].phrase_offsets, q[i].phrase_offsets + q[i].n_phrases + 1);
    last.tq_terms.emplace_back(q[i].terms, q[i].terms + q[i].phrase_offsets[q[i].n_phrases]);
    last.tq_mode.push_back(q[i].mode);
  }
}

// the counts every stub answers with: k, 0, 1 in turn, capped by k -- 0, 1 and k in one batch of three
int32_t count_of(int i, int top_k) { return std::min<int32_t>(i % 3 == 0 ? top_k : i % 3 == 1 ? 0 : 1, top_k); }
int64_t id_of(int i, int j) { return 1000 * (i + 1) + j; }
float score_of(int i, int j) { return (float)(i + 1) + (float)j / 64.f; }

int write_rows(int64_t* ids, float* sc, int32_t* cnt, int32_t B, int32_t top_k) {
  for (int i = 0; i < B; ++i) {
    cnt[i] = count_of(i, top_k);
    for (int j = 0; j < cnt[i]; ++j) {
      ids[(size_t)i * top_k + j] = id_of(i, j);
      sc[(size_t)i * top_k + j] = score_of(i, j);
    }
  }
  if (abandon && B > 0) cnt[0] = -1;
  abandon = false;
  return next_rc;
}
int members_of(int j, int g) { return j % 2 ? 1 : g; }
int write_groups(int64_t* ids, float* sc, int32_t* grp, int32_t* mem, int32_t* tot, int32_t* cnt, int32_t B, int32_t top_k, int32_t g) {
  last.with_scores = sc != nullptr;
  for (int i = 0; i < B; ++i) {
    cnt[i] = count_of(i, top_k);
    for (int j = 0; j < cnt[i]; ++j) {
      const size_t at = (size_t)i * top_k + j;
      grp[at] = 10 * i + j;
      mem[at] = members_of(j, g);
      tot[at] = members_of(j, g) + j;
      for (int m = 0; m < g; ++m) {
        ids[at * g + m] = id_of(i, m) + 10 * j;
        if (sc) sc[at * g + m] = score_of(i, m) + (float)j;
      }
    }
  }
  return next_rc;
}

}  // namespace

// ---- the stubs ----------------------------------------------------------------------------------------------------------
extern "C" {
const char* np_hip_last_error(void) { return MESSAGE; }
int np_hip_abi_version(void) { return NP_ABI_VERSION; }
int64_t np_hip_struct_size(int32_t which) { return which == 0 ? (int64_t)sizeof(np_info) : (int64_t)sizeof(np_stats); }
int np_hip_index_open(const char*, const np_open_opts*, np_index** out) {
  static int handle;
  *out = reinterpret_cast<np_index*>(&handle);
  return NP_OK;
}
void np_hip_index_close(np_index*) {}
int np_hip_index_info(const np_index*, np_info* out) {
  out->embedding_dim = DIM;
  out->num_documents = N_DOCS;
  return NP_OK;
}
int np_hip_index_probe_dir(const char*, np_info*) { return NP_ERR_IO; }

int np_hip_search_batch(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, const np_search_params* p,
                        const int64_t* subset, int64_t subset_len, int64_t* ids, float* sc, int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_batch");
  rec_queries(q, off, B, dim);
  r.p = *p;
  r.n_sub = subset_len;
  r.sub_null = subset == nullptr;
  if (subset) r.sub.assign(subset, subset + subset_len);
  return write_rows(ids, sc, cnt, B, p->top_k);
}
int np_hip_search_batch_subsets(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, const np_search_params* p,
                                const int64_t* sid, const int64_t* soff, int64_t n, const int32_t* qmap, int64_t* ids, float* sc,
                                int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_batch_subsets");
  rec_queries(q, off, B, dim);
  r.p = *p;
  rec_csr(sid, soff, n, qmap, B);
  return write_rows(ids, sc, cnt, B, p->top_k);
}
int np_hip_search_batch_filtered(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, const np_search_params* p,
                                 const np_filter* f, int32_t nf, const int32_t* qmap, int64_t* ids, float* sc, int32_t* cnt,
                                 np_stats*) {
  Recorded& r = begin("search_batch_filtered");
  rec_queries(q, off, B, dim);
  r.p = *p;
  rec_filters(f, nf);
  r.qmap.assign(qmap, qmap + B);
  return write_rows(ids, sc, cnt, B, p->top_k);
}
int np_hip_search_exact(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, int32_t top_k, int32_t precision,
                        const int64_t* sid, const int64_t* soff, int64_t n, const int32_t* qmap, int64_t* ids, float* sc,
                        int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_exact");
  rec_queries(q, off, B, dim);
  r.top_k = top_k;
  r.precision = precision;
  rec_csr(sid, soff, n, qmap, B);
  return write_rows(ids, sc, cnt, B, top_k);
}
int np_hip_search_exact_filtered(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, int32_t top_k,
                                 int32_t precision, const np_filter* f, int32_t nf, const int32_t* qmap, int64_t* ids, float* sc,
                                 int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_exact_filtered");
  rec_queries(q, off, B, dim);
  r.top_k = top_k;
  r.precision = precision;
  rec_filters(f, nf);
  r.qmap.assign(qmap, qmap + B);
  return write_rows(ids, sc, cnt, B, top_k);
}
int np_hip_text_search(const np_index*, const np_text_query* tq, int32_t B, int32_t top_k, const int64_t* sid, const int64_t* soff,
                       int64_t n, const int32_t* qmap, int64_t* ids, float* sc, int32_t* cnt, np_stats*) {
  Recorded& r = begin("text_search");
  r.B = B;
  r.top_k = top_k;
  rec_text(tq, B);
  rec_csr(sid, soff, n, qmap, B);
  return write_rows(ids, sc, cnt, B, top_k);
}
int np_hip_fuse(const np_index*, int32_t mode, float alpha, int32_t top_k, int32_t B, const int64_t* si, const float* ss,
                const int32_t* scnt, int32_t sw, const int64_t* ki, const float* ks, const int32_t* kcnt, int32_t kw, int64_t* ids,
                float* sc, int32_t* cnt) {
  Recorded& r = begin("fuse");
  r.fusion = mode;
  r.alpha = alpha;
  r.top_k = top_k;
  r.B = B;
  r.sem_w = sw;
  r.kw_w = kw;
  r.sem_ids.assign(si, si + (size_t)B * sw);
  r.sem_sc.assign(ss, ss + (size_t)B * sw);
  r.sem_cnt.assign(scnt, scnt + B);
  r.kw_ids.assign(ki, ki + (size_t)B * kw);
  r.kw_sc.assign(ks, ks + (size_t)B * kw);
  r.kw_cnt.assign(kcnt, kcnt + B);
  return write_rows(ids, sc, cnt, B, top_k);
}
int np_hip_search_hybrid(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, const np_search_params* p,
                         const np_text_query* tq, int32_t fetch_k, float alpha, int32_t fusion, const int64_t* sid,
                         const int64_t* soff, int64_t n, const int32_t* qmap, const np_filter* f, int32_t nf, int64_t* ids, float* sc,
                         int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_hybrid");
  rec_queries(q, off, B, dim);
  r.p = *p;
  rec_text(tq, B);
  r.fetch_k = fetch_k;
  r.alpha = alpha;
  r.fusion = fusion;
  rec_csr(sid, soff, n, qmap, B);
  rec_filters(f, nf);
  return write_rows(ids, sc, cnt, B, p->top_k);
}
int np_hip_collapse(const np_index*, int32_t top_k, int32_t group_size, int32_t B, const int64_t* li, const float* ls,
                    const int32_t* lc, int32_t w, int64_t* ids, float* sc, int32_t* grp, int32_t* mem, int32_t* tot, int32_t* cnt) {
  Recorded& r = begin("collapse");
  r.top_k = top_k;
  r.group_size = group_size;
  r.B = B;
  r.sem_w = w;
  r.sem_ids.assign(li, li + (size_t)B * w);
  if (ls) r.sem_sc.assign(ls, ls + (size_t)B * w);
  r.sem_cnt.assign(lc, lc + B);
  return write_groups(ids, sc, grp, mem, tot, cnt, B, top_k, group_size);
}
int np_hip_search_batch_grouped(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, const np_search_params* p,
                                const int64_t* sid, const int64_t* soff, int64_t n, const int32_t* qmap, const np_filter* f,
                                int32_t nf, int32_t pool_k, int32_t group_size, int64_t* ids, float* sc, int32_t* grp, int32_t* mem,
                                int32_t* tot, int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_batch_grouped");
  rec_queries(q, off, B, dim);
  r.p = *p;
  rec_csr(sid, soff, n, qmap, B);
  rec_filters(f, nf);
  r.pool_k = pool_k;
  r.group_size = group_size;
  return write_groups(ids, sc, grp, mem, tot, cnt, B, p->top_k, group_size);
}
int np_hip_search_hybrid_grouped(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim,
                                 const np_search_params* p, const np_text_query* tq, int32_t fetch_k, float alpha, int32_t fusion,
                                 const int64_t* sid, const int64_t* soff, int64_t n, const int32_t* qmap, const np_filter* f,
                                 int32_t nf, int32_t pool_k, int32_t group_size, int64_t* ids, float* sc, int32_t* grp, int32_t* mem,
                                 int32_t* tot, int32_t* cnt, np_stats*) {
  Recorded& r = begin("search_hybrid_grouped");
  rec_queries(q, off, B, dim);
  r.p = *p;
  rec_text(tq, B);
  r.fetch_k = fetch_k;
  r.alpha = alpha;
  r.fusion = fusion;
  rec_csr(sid, soff, n, qmap, B);
  rec_filters(f, nf);
  r.pool_k = pool_k;
  r.group_size = group_size;
  return write_groups(ids, sc, grp, mem, tot, cnt, B, p->top_k, group_size);
}
int np_hip_score_pairs(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, int32_t precision,
                       const int64_t* docs, const int64_t* poff, float* sc, float* sims, int32_t* pos, np_stats*) {
  Recorded& r = begin("score_pairs");
  rec_queries(q, off, B, dim);
  r.precision = precision;
  r.pair_off.assign(poff, poff + B + 1);
  r.pair_docs.assign(docs, docs + poff[B]);
  r.wants_matches = sims != nullptr && pos != nullptr;
  int64_t R = 0;
  for (int i = 0; i < B; ++i) R += (poff[i + 1] - poff[i]) * (off[i + 1] - off[i]);
  for (int64_t x = 0; x < poff[B]; ++x) sc[x] = (float)x + 0.5f;
  for (int64_t x = 0; sims && x < R; ++x) sims[x] = (float)x + 0.25f;
  for (int64_t x = 0; pos && x < R; ++x) pos[x] = (int32_t)x;
  return next_rc;
}
}  // extern "C"

namespace {
using namespace next_plaid;

struct Batch {   // query lengths 3, 1, 3 at dim 8, and what the library must see of them
  std::vector<std::vector<float>> rows;
  std::vector<Query> queries;
  std::vector<float> flat;
  std::vector<int32_t> off{0};
  explicit Batch(size_t n) {
    const size_t lens[3] = {3, 1, 3};
    for (size_t i = 0; i < n; ++i) {
      rows.emplace_back(lens[i] * DIM);
      for (size_t x = 0; x < rows[i].size(); ++x) rows[i][x] = (float)(100 * i + x);
      flat.insert(flat.end(), rows[i].begin(), rows[i].end());
      off.push_back(off.back() + (int32_t)lens[i]);
    }
    for (size_t i = 0; i < n; ++i) queries.push_back(Query{rows[i].data(), lens[i]});
  }
};

void check_queries(const Batch& b, size_t n) {
  CHECK(last.B == (int)n && last.dim == DIM && last.off == b.off && last.flat == b.flat);
}

void check_rows(const std::vector<QueryResult>& res, size_t n, size_t top_k) {
  CHECK(res.size() == n);
  for (size_t i = 0; i < res.size(); ++i) {
    const size_t c = (size_t)count_of((int)i, (int)top_k);
    CHECK(res[i].query_id == i && res[i].passage_ids.size() == c && res[i].scores.size() == c);
    for (size_t j = 0; j < c && j < res[i].passage_ids.size(); ++j)
      CHECK(res[i].passage_ids[j] == id_of((int)i, (int)j) && res[i].scores[j] == score_of((int)i, (int)j));
  }
}

void check_groups(const std::vector<MmapIndex::GroupedResult>& res, size_t n, size_t top_k, size_t g, bool scores) {
  CHECK(res.size() == n);
  for (size_t i = 0; i < res.size(); ++i) {
    CHECK(res[i].size() == (size_t)count_of((int)i, (int)top_k));
    for (size_t j = 0; j < res[i].size(); ++j) {
      const MmapIndex::Group& gr = res[i][j];
      const size_t m = (size_t)members_of((int)j, (int)g);
      CHECK(gr.group_id == (int32_t)(10 * i + j) && gr.total == (int32_t)(m + j) && gr.passage_ids.size() == m);
      CHECK(gr.scores.size() == (scores ? m : 0));
      for (size_t x = 0; x < gr.passage_ids.size(); ++x) {
        CHECK(gr.passage_ids[x] == id_of((int)i, (int)x) + 10 * (int64_t)j);
        if (scores) CHECK(gr.scores[x] == score_of((int)i, (int)x) + (float)j);
      }
    }
  }
}

// a shared object and a nullptr: query 0 and 2 share subset 0, query 1 has none
const std::vector<int64_t> SHARED{4, 2, 9};
std::vector<const std::vector<int64_t>*> subsets_of(size_t n) {
  std::vector<const std::vector<int64_t>*> s{&SHARED, nullptr, &SHARED};
  s.resize(n);
  return s;
}
void check_subsets(size_t n) {
  const std::vector<int32_t> qmap{0, -1, 0};
  CHECK(last.n_sub == (n ? 1 : 0) && last.qmap == std::vector<int32_t>(qmap.begin(), qmap.begin() + n));
  CHECK(last.soff == (n ? std::vector<int64_t>{0, 3} : std::vector<int64_t>{0}));
  CHECK(last.sid == (n ? SHARED : std::vector<int64_t>{}));
}
void check_no_subsets() {   // an empty vector of subsets means none: no CSR, no map
  CHECK(last.n_sub == 0 && last.qmap_null && last.sid.empty());
}
void check_no_filters() { CHECK(last.filters_null && last.n_filters == 0); }

std::vector<TextQuery> text_of(size_t n) {
  std::vector<TextQuery> t;
  t.push_back(TextQuery().phrase({3, 4}).phrase({7}));
  t.push_back(TextQuery().phrase({-1}));
  t.push_back(TextQuery(NP_TEXT_OR).phrase({9}));
  t.resize(n, TextQuery());
  return t;
}
void check_text(size_t n) {
  const std::vector<std::vector<int32_t>> terms{{3, 4, 7}, {-1}, {9}}, off{{0, 2, 3}, {0, 1}, {0, 1}};
  const std::vector<int32_t> mode{NP_TEXT_AND, NP_TEXT_AND, NP_TEXT_OR};
  CHECK(last.tq_terms == std::vector<std::vector<int32_t>>(terms.begin(), terms.begin() + n));
  CHECK(last.tq_off == std::vector<std::vector<int32_t>>(off.begin(), off.begin() + n));
  CHECK(last.tq_mode == std::vector<int32_t>(mode.begin(), mode.begin() + n));
}

size_t pool_k_default(size_t top_k, size_t limit) {
  return std::max<size_t>(1, std::min(std::min(std::max<size_t>(20 * top_k, 200), std::max<size_t>(N_DOCS, top_k)), limit));
}

template <class F>
bool throws(int kind, const char* text, F&& f) {
  try {
    f();
  } catch (const Error& e) {
    return e.kind == kind && std::string(e.what()).find(text) != std::string::npos;
  }
  return false;
}

void drive(const MmapIndex& ix, size_t n, size_t top_k) {
  const Batch b(n);
  SearchParameters params;
  params.top_k = top_k;
  params.n_full_scores = 77;
  params.n_ivf_probe = 3;
  params.centroid_score_threshold.reset();
  params.precision = 1;
  const std::vector<int64_t> subset{5, 1, 3};

  // search_batch: one subset for the batch stays on the one-subset entry, -1 = none
  check_rows(ix.search_batch(b.queries.data(), n, params, true), n, top_k);
  CHECK(last.entry == "search_batch" && last.sub_null && last.n_sub == -1);
  check_queries(b, n);
  CHECK(last.p.top_k == (int32_t)top_k && last.p.n_full_scores == 77 && last.p.n_ivf_probe == 3 && last.p.has_threshold == 0 &&
        last.p.centroid_score_threshold == 0.f && last.p.precision == 1 && last.p.centroid_batch_size == 100000);
  check_rows(ix.search_batch(b.queries.data(), n, params, false, &subset), n, top_k);
  CHECK(last.entry == "search_batch" && last.sub == subset && last.n_sub == 3);

  check_rows(ix.search_batch_subsets(b.queries.data(), n, params, true, subsets_of(n)), n, top_k);
  CHECK(last.entry == "search_batch_subsets" && last.p.top_k == (int32_t)top_k);
  check_queries(b, n);
  check_subsets(n);

  std::vector<FilterProgram> filters(1);
  filters[0].cmp(0, FilterProgram::GT, (int64_t)2000).is_null(0).or_();
  const std::vector<int32_t> qf_all{0, -1, 0}, qf(qf_all.begin(), qf_all.begin() + n);
  auto check_filters = [&] {
    CHECK(last.n_filters == 1 && last.filter_ops == std::vector<int32_t>({NP_F_CMP, NP_F_IS_NULL, NP_F_OR}));
    CHECK(last.filter_values == std::vector<std::vector<int64_t>>{{2000}} && last.qmap == qf);
  };
  check_rows(ix.search_batch_filtered(b.queries.data(), n, params, true, filters, qf), n, top_k);
  CHECK(last.entry == "search_batch_filtered");
  check_queries(b, n);
  check_filters();

  // the exact scans
  check_rows(ix.search_exact(b.queries.data(), n, top_k, 3), n, top_k);
  CHECK(last.entry == "search_exact" && last.top_k == (int)top_k && last.precision == 3 && last.n_sub == 0);
  CHECK(last.qmap == std::vector<int32_t>(n, -1) && last.soff == std::vector<int64_t>{0} && last.sid.empty());
  check_queries(b, n);
  check_rows(ix.search_exact(b.queries.data(), n, top_k, 0, &subset), n, top_k);
  CHECK(last.entry == "search_exact" && last.precision == 0 && last.n_sub == (n ? 1 : 0) && last.qmap == std::vector<int32_t>(n, 0));
  CHECK(last.sid == (n ? subset : std::vector<int64_t>{}));
  check_rows(ix.search_exact_subsets(b.queries.data(), n, top_k, 3, subsets_of(n)), n, top_k);
  CHECK(last.entry == "search_exact");
  check_queries(b, n);
  check_subsets(n);
  check_rows(ix.search_exact_filtered(b.queries.data(), n, top_k, 3, filters, qf), n, top_k);
  CHECK(last.entry == "search_exact_filtered" && last.top_k == (int)top_k && last.precision == 3);
  check_queries(b, n);
  check_filters();

  // keyword search and fusion
  check_rows(ix.text_search(text_of(n), top_k), n, top_k);
  CHECK(last.entry == "text_search" && last.B == (int)n && last.top_k == (int)top_k);
  check_text(n);
  check_no_subsets();
  check_rows(ix.text_search(text_of(n), top_k, subsets_of(n)), n, top_k);
  if (n) check_subsets(n);

  std::vector<QueryResult> sem(n), kw(n);
  if (n > 0) sem[0].passage_ids = {5, 6, 7}, sem[0].scores = {.5f, .25f, .125f}, kw[0].passage_ids = {6}, kw[0].scores = {3.f};
  if (n > 2) sem[2].passage_ids = {1}, sem[2].scores = {1.f}, kw[1].passage_ids = {8, 9}, kw[1].scores = {2.f, 1.f};
  check_rows(ix.fuse(NP_FUSE_RRF, 0.5f, top_k, sem, kw), n, top_k);
  const int sw = n ? 3 : 1, kww = n > 2 ? 2 : 1;
  CHECK(last.entry == "fuse" && last.fusion == NP_FUSE_RRF && last.alpha == 0.5f && last.top_k == (int)top_k && last.B == (int)n);
  CHECK(last.sem_w == sw && last.kw_w == kww);
  std::vector<int64_t> si(n * sw, 0), ki(n * kww, 0);
  std::vector<float> ss(n * sw, 0.f), ks(n * kww, 0.f);
  std::vector<int32_t> scnt(n, 0), kcnt(n, 0);
  for (size_t i = 0; i < n; ++i) {
    std::copy(sem[i].passage_ids.begin(), sem[i].passage_ids.end(), si.begin() + i * sw);
    std::copy(sem[i].scores.begin(), sem[i].scores.end(), ss.begin() + i * sw);
    std::copy(kw[i].passage_ids.begin(), kw[i].passage_ids.end(), ki.begin() + i * kww);
    std::copy(kw[i].scores.begin(), kw[i].scores.end(), ks.begin() + i * kww);
    scnt[i] = (int32_t)sem[i].passage_ids.size();
    kcnt[i] = (int32_t)kw[i].passage_ids.size();
  }
  CHECK(last.sem_ids == si && last.sem_sc == ss && last.sem_cnt == scnt && last.kw_ids == ki && last.kw_sc == ks && last.kw_cnt == kcnt);

  check_rows(ix.search_hybrid(b.queries.data(), text_of(n), params), n, top_k);
  CHECK(last.entry == "search_hybrid" && last.fetch_k == (int)(3 * top_k) && last.alpha == 0.75f && last.fusion == NP_FUSE_RELATIVE_SCORE);
  CHECK(last.p.top_k == (int32_t)top_k);
  check_queries(b, n);
  check_text(n);
  check_no_subsets();
  check_no_filters();
  check_rows(ix.search_hybrid(b.queries.data(), text_of(n), params, 0.25f, NP_FUSE_RRF, 11, subsets_of(n)), n, top_k);
  CHECK(last.fetch_k == 11 && last.alpha == 0.25f && last.fusion == NP_FUSE_RRF);
  if (n) check_subsets(n);

  // grouped search
  for (size_t g : {1, 2}) {
    for (bool scores : {true, false}) {
      check_groups(ix.collapse(sem, top_k, g, scores), n, top_k, g, scores);
      CHECK(last.entry == "collapse" && last.top_k == (int)top_k && last.group_size == (int)g && last.B == (int)n && last.sem_w == sw);
      CHECK(last.sem_ids == si && last.sem_cnt == scnt && last.with_scores == scores && last.sem_sc == (scores ? ss : std::vector<float>{}));
    }
    check_groups(ix.search_grouped(b.queries.data(), n, params, g), n, top_k, g, true);
    CHECK(last.entry == "search_batch_grouped" && last.pool_k == (int)pool_k_default(top_k, NP_GROUP_MAX_LIST) && last.group_size == (int)g);
    CHECK(last.p.top_k == (int32_t)top_k);
    check_queries(b, n);
    check_no_subsets();
    check_no_filters();
    check_groups(ix.search_grouped(b.queries.data(), n, params, g, 33, subsets_of(n)), n, top_k, g, true);
    CHECK(last.pool_k == 33);
    if (n) check_subsets(n);

    check_groups(ix.search_hybrid_grouped(b.queries.data(), text_of(n), params, g), n, top_k, g, true);
    const size_t pk = pool_k_default(top_k, 2 * NP_TEXT_MAX_TOPK);
    CHECK(last.entry == "search_hybrid_grouped" && last.pool_k == (int)pk && last.fetch_k == (int)std::min<size_t>(3 * pk, NP_TEXT_MAX_TOPK));
    CHECK(last.group_size == (int)g && last.alpha == 0.75f && last.fusion == NP_FUSE_RELATIVE_SCORE && last.p.top_k == (int32_t)top_k);
    check_queries(b, n);
    check_text(n);
    check_no_subsets();
    check_no_filters();
    check_groups(ix.search_hybrid_grouped(b.queries.data(), text_of(n), params, g, 40, 0.5f, NP_FUSE_RRF, 9, subsets_of(n)), n, top_k, g, true);
    CHECK(last.pool_k == 40 && last.fetch_k == 9 && last.alpha == 0.5f && last.fusion == NP_FUSE_RRF);
    if (n) check_subsets(n);
  }

  // given pairs: an empty list of documents for one query
  const std::vector<std::vector<int64_t>> all_docs{{4, 4, 2}, {}, {9}}, docs(all_docs.begin(), all_docs.begin() + n);
  for (bool matches : {true, false}) {
    const auto out = ix.score_pairs(b.queries.data(), n, docs, matches, 0);
    CHECK(last.entry == "score_pairs" && last.precision == 0 && last.wants_matches == matches && out.size() == n);
    check_queries(b, n);
    std::vector<int64_t> poff{0}, flat_docs;
    for (const auto& d : docs) {
      flat_docs.insert(flat_docs.end(), d.begin(), d.end());
      poff.push_back((int64_t)flat_docs.size());
    }
    CHECK(last.pair_off == poff && last.pair_docs == flat_docs);
    size_t p0 = 0, r0 = 0;
    for (size_t i = 0; i < out.size(); ++i) {
      const size_t ni = docs[i].size(), rows = ni * b.queries[i].n_tokens;
      CHECK(out[i].scores.size() == ni && out[i].token_sims.size() == (matches ? rows : 0) && out[i].token_pos.size() == out[i].token_sims.size());
      for (size_t x = 0; x < out[i].scores.size(); ++x) CHECK(out[i].scores[x] == (float)(p0 + x) + 0.5f);
      for (size_t x = 0; x < out[i].token_sims.size(); ++x)
        CHECK(out[i].token_sims[x] == (float)(r0 + x) + 0.25f && out[i].token_pos[x] == (int32_t)(r0 + x));
      p0 += ni;
      r0 += rows;
    }
  }

  // one entry per query, the message prefixed with the method's name; nothing reaches the library
  const int before = n_calls;
  const auto wrong = subsets_of(n + 1);
  const std::vector<int32_t> wrong_qf(n + 1, 0);
  auto refused = [&](const char* text, auto&& call) { CHECK(throws(NP_ERR_INVALID_ARGUMENT, text, call)); };
  const Query* qp = b.queries.data();
  refused("search_batch_subsets: one subset entry per query", [&] { ix.search_batch_subsets(qp, n, params, true, wrong); });
  refused("search_exact_subsets: one subset entry per query", [&] { ix.search_exact_subsets(qp, n, top_k, 0, wrong); });
  refused("text_search: one subset entry per query", [&] { ix.text_search(text_of(n), top_k, wrong); });
  refused("search_hybrid: one subset entry per query",
          [&] { ix.search_hybrid(qp, text_of(n), params, 0.75f, NP_FUSE_RRF, 0, wrong); });
  refused("search_grouped: one subset entry per query", [&] { ix.search_grouped(qp, n, params, 1, 0, wrong); });
  refused("search_hybrid_grouped: one subset entry per query",
          [&] { ix.search_hybrid_grouped(qp, text_of(n), params, 1, 0, 0.75f, NP_FUSE_RRF, 0, wrong); });
  refused("search_batch_filtered: one query_filter entry per query",
          [&] { ix.search_batch_filtered(qp, n, params, true, filters, wrong_qf); });
  refused("search_exact_filtered: one query_filter entry per query",
          [&] { ix.search_exact_filtered(qp, n, top_k, 0, filters, wrong_qf); });
  refused("fuse: one keyword list per semantic list", [&] { ix.fuse(NP_FUSE_RRF, 0.5f, top_k, sem, std::vector<QueryResult>(n + 1)); });
  refused("score_pairs: one list of document ids per query",
          [&] { ix.score_pairs(qp, n, std::vector<std::vector<int64_t>>(n + 1)); });
  CHECK(n_calls == before);

  // the run_batch policy: NP_ERR_SEARCH under `parallel` gives empty results, anything else throws, a negative count throws
  auto batch_forms = [&](bool parallel, auto&& verdict) {
    verdict([&] { return ix.search_batch(b.queries.data(), n, params, parallel); });
    verdict([&] { return ix.search_batch_subsets(b.queries.data(), n, params, parallel, subsets_of(n)); });
    verdict([&] { return ix.search_batch_filtered(b.queries.data(), n, params, parallel, filters, qf); });
  };
  next_rc = NP_ERR_SEARCH;
  batch_forms(true, [&](auto&& call) {
    const auto res = call();
    CHECK(res.size() == n);
    for (size_t i = 0; i < res.size(); ++i) CHECK(res[i].query_id == i && res[i].passage_ids.empty() && res[i].scores.empty());
  });
  batch_forms(false, [&](auto&& call) { CHECK(throws(NP_ERR_SEARCH, MESSAGE, call)); });
  next_rc = NP_ERR_SHAPE;
  batch_forms(true, [&](auto&& call) { CHECK(throws(NP_ERR_SHAPE, MESSAGE, call)); });
  // ... and every other entry throws the library's error whatever it is
  next_rc = NP_ERR_SEARCH;
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search_exact(b.queries.data(), n, top_k); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search_exact_filtered(b.queries.data(), n, top_k, 0, filters, qf); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.text_search(text_of(n), top_k); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.fuse(NP_FUSE_RRF, 0.5f, top_k, sem, kw); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search_hybrid(b.queries.data(), text_of(n), params); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.collapse(sem, top_k, 1); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search_grouped(b.queries.data(), n, params); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search_hybrid_grouped(b.queries.data(), text_of(n), params); }));
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.score_pairs(b.queries.data(), n, docs); }));
  next_rc = NP_OK;
  if (n) {
    batch_forms(true, [&](auto&& call) {
      abandon = true;
      CHECK(throws(NP_ERR_SEARCH, "the batch was abandoned", call));
    });
  }
}

}  // namespace

int main() {
  unsetenv("NEXT_PLAID_FORCE_CPU");
  unsetenv("NEXT_PLAID_FORCE_GPU");
  MmapIndex ix = MmapIndex::load("an/index");
  CHECK(ix.on_device() && ix.embedding_dim() == (size_t)DIM && ix.num_documents() == (size_t)N_DOCS);
  for (size_t n : {0, 1, 3})
    for (size_t top_k : {0, 1, 5}) drive(ix, n, top_k);
  // search(): the batch of one without the parallel policy, query_id 0
  const Batch one(1);
  SearchParameters params;
  params.top_k = 5;
  const QueryResult r = ix.search(one.rows[0].data(), 3, params);
  CHECK(last.entry == "search_batch" && last.B == 1 && r.query_id == 0 && r.passage_ids.size() == 5);
  CHECK(last.p.has_threshold == 1 && last.p.centroid_score_threshold == 0.4f && last.p.precision == 2);
  next_rc = NP_ERR_SEARCH;
  CHECK(throws(NP_ERR_SEARCH, MESSAGE, [&] { ix.search(one.rows[0].data(), 3, params); }));
  next_rc = NP_OK;
  if (failed) {
    std::printf("%d checks FAILED\n", failed);
    return 1;
  }
  std::printf("all checks passed (%d calls)\n", n_calls);
  return 0;
}
