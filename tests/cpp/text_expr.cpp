// Tree queries (next_plaid::TextExpr) through next_plaid.hpp on an index directory:
//   text_expr <index_dir> <term_offsets.i64> <inst_doc.i64> <inst_pos.i32> <n_rows> <queries.f32> <lens.i64>
// The arguments are text_hybrid.cpp's.  Text query i is, over term ids: i % 3 == 0: (0 OR 1) NOT 2;  1: "2 3" OR 1* with the
// prefix standing for the terms [1, 4);  2: (0 AND -1) OR 4.  Query i is scoped to the even document ids below 60 when
// i % 2 == 1.  Prints, per stage, one line per query:
//   <stage> <query> <count> then <id>:<score bits, hex> per hit
// for text_search (top 9) and search_hybrid (relative score, alpha 0.75, top 5 of 15).  tests/test_gpu_text_expr.py compares
// the lines with the Python calls.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "next_plaid.hpp"

template <class T>
static std::vector<T> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
  return v;
}

static void print(const char* stage, const std::vector<next_plaid::QueryResult>& res) {
  for (const auto& r : res) {
    std::printf("%s %zu %zu", stage, (size_t)r.query_id, r.passage_ids.size());
    for (size_t j = 0; j < r.passage_ids.size(); ++j) {
      uint32_t bits;
      std::memcpy(&bits, &r.scores[j], 4);
      std::printf(" %lld:%08x", (long long)r.passage_ids[j], bits);
    }
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 8) {
    std::fprintf(stderr, "usage: %s index_dir term_offsets.i64 inst_doc.i64 inst_pos.i32 n_rows queries.f32 lens.i64\n", argv[0]);
    return 2;
  }
  try {
    next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(argv[1]);
    const std::vector<int64_t> toff = read_all<int64_t>(argv[2]), idoc = read_all<int64_t>(argv[3]);
    const std::vector<int32_t> ipos = read_all<int32_t>(argv[4]);
    const next_plaid::TextIndexSpan span{toff.data(), toff.size() - 1, idoc.data(), ipos.data(), std::atoll(argv[5])};
    ix.set_text(&span);
    const std::vector<float> rows = read_all<float>(argv[6]);
    const std::vector<int64_t> lens = read_all<int64_t>(argv[7]);
    const size_t dim = ix.embedding_dim();
    std::vector<next_plaid::Query> qs;
    std::vector<next_plaid::TextExpr> tq;
    size_t at = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
      qs.push_back({rows.data() + at * dim, (size_t)lens[i]});
      at += (size_t)lens[i];
      next_plaid::TextExpr e;
      if (i % 3 == 0) {
        const int a = e.phrase({0}), b = e.phrase({1}), l = e.or_(a, b);
        e.not_(l, e.phrase({2}));
      } else if (i % 3 == 1) {
        const int a = e.phrase({2, 3}), b = e.phrase({1}, 4);
        e.or_(a, b);
      } else {
        const int a = e.phrase({0}), b = e.phrase({-1}), l = e.and_(a, b);
        e.or_(l, e.phrase({4}));
      }
      tq.push_back(e);
    }
    std::vector<int64_t> evens;
    for (int64_t d = 0; d < 60; d += 2) evens.push_back(d);
    std::vector<const std::vector<int64_t>*> subsets(qs.size(), nullptr);
    for (size_t i = 0; i < qs.size(); ++i) subsets[i] = i % 2 == 1 ? &evens : nullptr;
    print("text", ix.text_search(tq, 9, subsets));
    next_plaid::SearchParameters p;
    p.top_k = 5;
    p.n_full_scores = 64;
    p.n_ivf_probe = 4;
    print("hybrid", ix.search_hybrid(qs.data(), tq, p, 0.75f, NP_FUSE_RELATIVE_SCORE, 15, subsets));
    ix.set_text(nullptr);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "text_expr: %s\n", e.what());
    return 1;
  }
  return 0;
}
