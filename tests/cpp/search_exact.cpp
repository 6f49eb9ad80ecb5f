// Exact search through next_plaid.hpp (MmapIndex::search_exact_subsets) on an index directory:
//   search_exact <index_dir> <queries.f32> <lens.i64> <top_k> <precision>
// The queries' token rows are concatenated in queries.f32; lens.i64 holds their lengths.  Query i searches the even document
// ids below 60 when i % 3 == 1, ids 3..9 when i % 3 == 2, and everything otherwise.  Prints one line per query:
//   <query> <count> then <id>:<score bits, hex> per hit
// tests/test_gpu_scan.py compares the lines with the Python call.
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

int main(int argc, char** argv) {
  if (argc != 6) {
    std::fprintf(stderr, "usage: %s index_dir queries.f32 lens.i64 top_k precision\n", argv[0]);
    return 2;
  }
  try {
    next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(argv[1]);
    const std::vector<float> rows = read_all<float>(argv[2]);
    const std::vector<int64_t> lens = read_all<int64_t>(argv[3]);
    const size_t dim = ix.embedding_dim();
    std::vector<next_plaid::Query> qs;
    size_t at = 0;
    for (int64_t n : lens) {
      qs.push_back({rows.data() + at * dim, (size_t)n});
      at += (size_t)n;
    }
    std::vector<int64_t> evens, few;
    for (int64_t d = 0; d < 60; d += 2) evens.push_back(d);
    for (int64_t d = 3; d < 10; ++d) few.push_back(d);
    std::vector<const std::vector<int64_t>*> subsets(qs.size(), nullptr);
    for (size_t i = 0; i < qs.size(); ++i) subsets[i] = i % 3 == 1 ? &evens : i % 3 == 2 ? &few : nullptr;
    const auto res = ix.search_exact_subsets(qs.data(), qs.size(), (size_t)std::atoll(argv[4]), std::atoi(argv[5]), subsets);
    for (const auto& r : res) {
      std::printf("%zu %zu", (size_t)r.query_id, r.passage_ids.size());
      for (size_t j = 0; j < r.passage_ids.size(); ++j) {
        uint32_t bits;
        std::memcpy(&bits, &r.scores[j], 4);
        std::printf(" %lld:%08x", (long long)r.passage_ids[j], bits);
      }
      std::printf("\n");
    }
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
