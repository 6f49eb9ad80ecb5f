// What next_plaid.hpp's TextExpr and the text_search / search_hybrid overloads that take it hand the library -- with the host
// compiler alone.  The np_hip_* entries the header reaches are recording stubs in this translation unit (no library is
// linked; member functions that are not called are never emitted).  Checked: which entry a tree query reaches and which a
// flat one, the phrases, prefix ranges and nodes behind the struct, the scope and the rows that come back.
// Built with -fsanitize=address,undefined: an array the header sized too small is an error here.
#include <cstdio>
#include <string>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

namespace {

constexpr int DIM = 4;
int failed = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failed;                                                  \
    }                                                            \
  } while (0)

struct Tree {
  std::vector<int32_t> terms, off, hi, nodes;   // nodes as op, a, b triples
  bool operator==(const Tree& o) const { return terms == o.terms && off == o.off && hi == o.hi && nodes == o.nodes; }
};
std::string entry;
std::vector<Tree> trees;
std::vector<int32_t> flat_modes, qmap;
std::vector<int64_t> sid, soff;
int B = -1, top_k = -1, fetch_k = -1, fusion = -1, n_filters = -1;
float alpha = -1.f;
int next_rc = NP_OK;

void rec_exprs(const np_text_expr* q, int32_t n) {
  trees.clear();
  for (int32_t i = 0; i < n; ++i) {
    Tree t;
    t.off.assign(q[i].phrase_offsets, q[i].phrase_offsets + q[i].n_phrases + 1);
    t.terms.assign(q[i].terms, q[i].terms + t.off.back());
    t.hi.assign(q[i].prefix_hi, q[i].prefix_hi + q[i].n_phrases);
    for (int32_t x = 0; x < q[i].n_nodes; ++x) {
      t.nodes.push_back(q[i].nodes[x].op);
      t.nodes.push_back(q[i].nodes[x].a);
      t.nodes.push_back(q[i].nodes[x].b);
    }
    trees.push_back(t);
  }
}
void rec_csr(const int64_t* s, const int64_t* o, int64_t n, const int32_t* m, int32_t n_q) {
  soff.clear(), sid.clear(), qmap.clear();   // (no scope: NULL arrays and n = 0)
  if (o) soff.assign(o, o + n + 1);
  if (s && o) sid.assign(s, s + o[n]);
  if (m) qmap.assign(m, m + n_q);
}
int write_rows(int64_t* ids, float* sc, int32_t* cnt, int32_t n, int32_t k) {
  for (int i = 0; i < n; ++i) {
    cnt[i] = i % 2 ? 0 : k;
    for (int j = 0; j < cnt[i]; ++j) {
      ids[(size_t)i * k + j] = 100 * (i + 1) + j;
      sc[(size_t)i * k + j] = (float)(i + 1) + (float)j / 8.f;
    }
  }
  return next_rc;
}

}  // namespace

extern "C" {
const char* np_hip_last_error(void) { return "Invalid argument: the stub said so"; }
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
  out->num_documents = 50;
  return NP_OK;
}
int np_hip_index_probe_dir(const char*, np_info*) { return NP_ERR_IO; }

int np_hip_text_search(const np_index*, const np_text_query* tq, int32_t n, int32_t k, const int64_t* s, const int64_t* o, int64_t ns,
                       const int32_t* m, int64_t* ids, float* sc, int32_t* cnt, np_stats*) {
  entry = "text_search";
  B = n, top_k = k;
  flat_modes.clear();
  for (int32_t i = 0; i < n; ++i) flat_modes.push_back(tq[i].mode);
  rec_csr(s, o, ns, m, n);
  return write_rows(ids, sc, cnt, n, k);
}
int np_hip_text_search_expr(const np_index*, const np_text_expr* tq, int32_t n, int32_t k, const int64_t* s, const int64_t* o,
                            int64_t ns, const int32_t* m, int64_t* ids, float* sc, int32_t* cnt, np_stats*) {
  entry = "text_search_expr";
  B = n, top_k = k;
  rec_exprs(tq, n);
  rec_csr(s, o, ns, m, n);
  return write_rows(ids, sc, cnt, n, k);
}
int np_hip_search_hybrid_expr(const np_index*, const float*, const int32_t* off, int32_t n, int32_t dim, const np_search_params* p,
                              const np_text_expr* tq, int32_t fk, float a, int32_t f, const int64_t* s, const int64_t* o, int64_t ns,
                              const int32_t* m, const np_filter* filters, int32_t nf, int64_t* ids, float* sc, int32_t* cnt, np_stats*) {
  entry = "search_hybrid_expr";
  B = n, top_k = p->top_k, fetch_k = fk, alpha = a, fusion = f;
  n_filters = filters ? nf : -1;
  if (dim != DIM || off[n] != 3 * n) ++failed;
  rec_exprs(tq, n);
  rec_csr(s, o, ns, m, n);
  return write_rows(ids, sc, cnt, n, p->top_k);
}
}

using namespace next_plaid;

int main() {
  MmapIndex ix = MmapIndex::load("an/index");
  // (7 OR "8 9") NOT 3*   with the prefix standing for the terms [3, 6);  a single phrase;  5 AND 6
  TextExpr a, b, c;
  const int a0 = a.phrase({7}), a1 = a.phrase({8, 9}), l = a.or_(a0, a1);
  CHECK(a.not_(l, a.phrase({3}, 6)) == 4);
  b.phrase({-1});
  const int c0 = c.phrase({5}), c1 = c.phrase({6});
  c.and_(c0, c1);
  const Tree ta{{7, 8, 9, 3}, {0, 1, 3, 4}, {0, 0, 6},
                {NP_TEXT_NODE_PHRASE, 0, 0, NP_TEXT_NODE_PHRASE, 1, 0, NP_TEXT_NODE_OR, 0, 1, NP_TEXT_NODE_PHRASE, 2, 0, NP_TEXT_NODE_NOT, 2, 3}};
  const Tree tb{{-1}, {0, 1}, {0}, {NP_TEXT_NODE_PHRASE, 0, 0}};
  const Tree tc{{5, 6}, {0, 1, 2}, {0, 0}, {NP_TEXT_NODE_PHRASE, 0, 0, NP_TEXT_NODE_PHRASE, 1, 0, NP_TEXT_NODE_AND, 0, 1}};
  const std::vector<int64_t> some = {4, 8, 15};
  {   // trees reach the _expr entry with their arrays; the rows come back at their stride
    const std::vector<QueryResult> r = ix.text_search(std::vector<TextExpr>{a, b, c}, 3, {nullptr, &some, &some});
    CHECK(entry == "text_search_expr" && B == 3 && top_k == 3);
    CHECK(trees.size() == 3 && trees[0] == ta && trees[1] == tb && trees[2] == tc);
    CHECK((qmap == std::vector<int32_t>{-1, 0, 0}) && sid == some && (soff == std::vector<int64_t>{0, 3}));
    CHECK(r.size() == 3 && r[0].passage_ids.size() == 3 && r[1].passage_ids.empty() && r[2].passage_ids.size() == 3);
    CHECK(r[2].query_id == 2 && r[2].passage_ids[1] == 301 && r[2].scores[1] == 3.125f);
  }
  {   // flat queries keep their entry
    ix.text_search(std::vector<TextQuery>{TextQuery(NP_TEXT_OR).phrase({1}).phrase({2})}, 2);
    CHECK(entry == "text_search" && B == 1 && (flat_modes == std::vector<int32_t>{NP_TEXT_OR}));
  }
  {   // the hybrid request
    const std::vector<float> rows(2 * 3 * DIM, 0.5f);
    const Query qs[2] = {{rows.data(), 3}, {rows.data() + 3 * DIM, 3}};
    SearchParameters p;
    p.top_k = 4;
    const std::vector<QueryResult> r = ix.search_hybrid(qs, std::vector<TextExpr>{c, a}, p, 0.25f, NP_FUSE_RRF, 0, {&some, nullptr});
    CHECK(entry == "search_hybrid_expr" && B == 2 && top_k == 4 && fetch_k == 12 && alpha == 0.25f && fusion == NP_FUSE_RRF);
    CHECK(n_filters == -1 && trees.size() == 2 && trees[0] == tc && trees[1] == ta && (qmap == std::vector<int32_t>{0, -1}));
    CHECK(r.size() == 2 && r[0].passage_ids.size() == 4 && r[1].passage_ids.empty());
    ix.search_hybrid(qs, std::vector<TextExpr>{c, a}, p, 0.75f, NP_FUSE_RELATIVE_SCORE, 9);
    CHECK(fetch_k == 9 && fusion == NP_FUSE_RELATIVE_SCORE && qmap.empty() && soff.empty());
  }
  {   // a refusal is the mapped error with the library's message
    next_rc = NP_ERR_INVALID_ARGUMENT;
    try {
      ix.text_search(std::vector<TextExpr>{a}, 3);
      CHECK(!"no throw");
    } catch (const Error& e) {
      CHECK(e.kind == Error::Config && std::string(e.what()) == "Invalid argument: the stub said so");
    }
    next_rc = NP_OK;
  }
  if (failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
