// Given pairs through next_plaid.hpp (MmapIndex::score_pairs) on an index directory:
//   score_pairs <index_dir> <queries.f32> <lens.i64> <pair_docs.i64> <pair_counts.i64>
// The queries' token rows are concatenated in queries.f32 and lens.i64 holds their lengths; pair_docs.i64 holds the
// document ids of all pairs, query by query, and pair_counts.i64 how many each query has.  Prints one line per pair:
//   <query> <document> <score bits, hex> then <sim bits, hex>:<position> per query token
// tests/test_gpu_pairs.py compares the lines with the Python call.
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

static uint32_t bits_of(float x) {
  uint32_t b;
  std::memcpy(&b, &x, 4);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s index_dir queries.f32 lens.i64 pair_docs.i64 pair_counts.i64\n", argv[0]);
    return 2;
  }
  try {
    next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(argv[1]);
    const std::vector<float> rows = read_all<float>(argv[2]);
    const std::vector<int64_t> lens = read_all<int64_t>(argv[3]);
    const std::vector<int64_t> docs = read_all<int64_t>(argv[4]);
    const std::vector<int64_t> counts = read_all<int64_t>(argv[5]);
    if (counts.size() != lens.size()) {
      std::fprintf(stderr, "one pair count per query\n");
      return 2;
    }
    const size_t dim = ix.embedding_dim();
    std::vector<next_plaid::Query> qs;
    std::vector<std::vector<int64_t>> ids;
    size_t at = 0, dat = 0;
    for (size_t i = 0; i < lens.size(); ++i) {
      qs.push_back({rows.data() + at * dim, (size_t)lens[i]});
      at += (size_t)lens[i];
      ids.emplace_back(docs.begin() + dat, docs.begin() + dat + counts[i]);
      dat += (size_t)counts[i];
    }
    const auto res = ix.score_pairs(qs.data(), qs.size(), ids);
    for (size_t i = 0; i < res.size(); ++i) {
      const size_t lq = qs[i].n_tokens;
      for (size_t p = 0; p < ids[i].size(); ++p) {
        std::printf("%zu %lld %08x", i, (long long)ids[i][p], bits_of(res[i].scores[p]));
        for (size_t t = 0; t < lq; ++t)
          std::printf(" %08x:%d", bits_of(res[i].token_sims[p * lq + t]), (int)res[i].token_pos[p * lq + t]);
        std::printf("\n");
      }
    }
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
