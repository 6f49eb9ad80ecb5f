// Keyword search, fusion and the hybrid request through next_plaid.hpp on an index directory:
//   text_hybrid <index_dir> <term_offsets.i64> <inst_doc.i64> <inst_pos.i32> <n_rows> <queries.f32> <lens.i64>
// The keyword index is the three arrays; the queries' token rows are concatenated in queries.f32, lens.i64 holds their
// lengths.  Text query i is, over term ids: i % 3 == 0: [0] AND [1];  1: [2, 3] (a phrase) OR [1];  2: [0] OR [-1] OR [4].
// Query i is scoped to the even document ids below 60 when i % 2 == 1.  Prints, per stage, one line per query:
//   <stage> <query> <count> then <id>:<score bits, hex> per hit
// for text_search (top 9), search_hybrid (relative score, alpha 0.75, top 5 of 15) and the fusion (rrf, alpha 0.5) of the
// keyword list with itself reversed.  tests/test_gpu_text.py compares the lines with the Python calls.
#include <algorithm>
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
    std::vector<next_plaid::TextQuery> tq;
    size_t at = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
      qs.push_back({rows.data() + at * dim, (size_t)lens[i]});
      at += (size_t)lens[i];
      if (i % 3 == 0) tq.push_back(next_plaid::TextQuery(NP_TEXT_AND).phrase({0}).phrase({1}));
      else if (i % 3 == 1) tq.push_back(next_plaid::TextQuery(NP_TEXT_OR).phrase({2, 3}).phrase({1}));
      else tq.push_back(next_plaid::TextQuery(NP_TEXT_OR).phrase({0}).phrase({-1}).phrase({4}));
    }
    std::vector<int64_t> evens;
    for (int64_t d = 0; d < 60; d += 2) evens.push_back(d);
    std::vector<const std::vector<int64_t>*> subsets(qs.size(), nullptr);
    for (size_t i = 0; i < qs.size(); ++i) subsets[i] = i % 2 == 1 ? &evens : nullptr;
    const auto kw = ix.text_search(tq, 9, subsets);
    print("text", kw);
    next_plaid::SearchParameters p;
    p.top_k = 5;
    p.n_full_scores = 64;
    p.n_ivf_probe = 4;
    print("hybrid", ix.search_hybrid(qs.data(), tq, p, 0.75f, NP_FUSE_RELATIVE_SCORE, 15, subsets));
    auto rev = kw;
    for (auto& r : rev) {
      std::reverse(r.passage_ids.begin(), r.passage_ids.end());
      std::reverse(r.scores.begin(), r.scores.end());
    }
    print("fuse", ix.fuse(NP_FUSE_RRF, 0.5f, 6, kw, rev));
    ix.set_text(nullptr);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
