// Grouped search through next_plaid.hpp on an index directory:
//   search_grouped <index_dir> <term_offsets.i64> <inst_doc.i64> <inst_pos.i32> <n_rows> <queries.f32> <lens.i64> <groups.i32>
// The keyword index is the three arrays; the queries' token rows are concatenated in queries.f32, lens.i64 holds their
// lengths; groups.i32 holds one dense group id per document.  Text query i is, over term ids: i % 3 == 0: [0] AND [1];
// 1: [2, 3] (a phrase) OR [1];  2: [0] OR [-1] OR [4].  Query i is scoped to the even document ids below 60 when i % 2 == 1.
// Prints, per stage, one line per query:
//   <stage> <query> <groups> then per group: | <group id> <total> and <id>:<score bits, hex> per member
// for search_grouped (top 3 groups of 2 out of a pool of 30), search_hybrid_grouped (relative score, alpha 0.75, pool 24 of
// fetch 15) and the collapse (top 2 groups of 3) of an unscoped search_batch of 20.  tests/test_gpu_grouped.py compares the
// lines with the Python calls.
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

static void print(const char* stage, const std::vector<next_plaid::MmapIndex::GroupedResult>& res) {
  for (size_t i = 0; i < res.size(); ++i) {
    std::printf("%s %zu %zu", stage, i, res[i].size());
    for (const auto& g : res[i]) {
      std::printf(" | %d %d", g.group_id, g.total);
      for (size_t j = 0; j < g.passage_ids.size(); ++j) {
        uint32_t bits;
        std::memcpy(&bits, &g.scores[j], 4);
        std::printf(" %lld:%08x", (long long)g.passage_ids[j], bits);
      }
    }
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s index_dir term_offsets.i64 inst_doc.i64 inst_pos.i32 n_rows queries.f32 lens.i64 groups.i32\n",
                 argv[0]);
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
    const std::vector<int32_t> groups = read_all<int32_t>(argv[8]);
    int32_t n_groups = 0;
    for (int32_t g : groups) n_groups = g + 1 > n_groups ? g + 1 : n_groups;
    ix.set_groups(groups, n_groups);
    if (ix.group_count() != n_groups) return 3;
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
    next_plaid::SearchParameters p;
    p.top_k = 3;
    p.n_full_scores = 64;
    p.n_ivf_probe = 4;
    print("grouped", ix.search_grouped(qs.data(), qs.size(), p, 2, 30, subsets));
    print("hybrid", ix.search_hybrid_grouped(qs.data(), tq, p, 2, 24, 0.75f, NP_FUSE_RELATIVE_SCORE, 15, subsets));
    next_plaid::SearchParameters wide = p;
    wide.top_k = 20;
    print("collapse", ix.collapse(ix.search_batch(qs.data(), qs.size(), wide, true), 2, 3));
    ix.set_groups({}, 0);
    if (ix.group_count() != 0) return 3;
    ix.set_text(nullptr);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
