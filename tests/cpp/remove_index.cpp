// The C++ mirror's resident remove on a real device (tests/test_gpu_index_remove.py builds it against libnextplaid_hip.so):
//   remove_index <index_dir> <ids.i64> <queries.f32> <n_queries> <tokens_per_query>
// loads the directory, searches, remove()s the listed ids -- the directory and the handle -- and searches again on the same
// handle.  Prints "removed <n> documents <left>" and one JSON line per query and state ("before" / "after").
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "next_plaid.hpp"

namespace {
template <class T>
std::vector<T> read_all(const char* path) {
  std::vector<T> v;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path);
    std::exit(2);
  }
  T x;
  while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
void print_rows(const char* state, const std::vector<next_plaid::QueryResult>& res) {
  for (const auto& r : res) {
    std::printf("{\"state\": \"%s\", \"query_id\": %zu, \"passage_ids\": [", state, r.query_id);
    for (size_t j = 0; j < r.passage_ids.size(); ++j) std::printf("%s%lld", j ? ", " : "", (long long)r.passage_ids[j]);
    std::printf("], \"scores\": [");
    for (size_t j = 0; j < r.scores.size(); ++j) std::printf("%s%.9g", j ? ", " : "", r.scores[j]);
    std::printf("]}\n");
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s index_dir ids.i64 queries.f32 n_queries tokens_per_query\n", argv[0]);
    return 2;
  }
  try {
    auto index = next_plaid::MmapIndex::load(argv[1]);
    const std::vector<int64_t> ids = read_all<int64_t>(argv[2]);
    const std::vector<float> buf = read_all<float>(argv[3]);
    const size_t nq = std::strtoul(argv[4], nullptr, 10), lq = std::strtoul(argv[5], nullptr, 10), dim = index.embedding_dim();
    if (buf.size() != nq * lq * dim) {
      std::fprintf(stderr, "%s holds %zu floats, not %zu\n", argv[3], buf.size(), nq * lq * dim);
      return 2;
    }
    next_plaid::SearchParameters p;
    p.top_k = 10, p.n_ivf_probe = 8, p.n_full_scores = 128;
    std::vector<next_plaid::Query> qs(nq);
    for (size_t i = 0; i < nq; ++i) qs[i] = {buf.data() + i * lq * dim, lq};
    print_rows("before", index.search_batch(qs.data(), nq, p, /*parallel=*/true));
    const long long n = (long long)index.remove(ids);
    std::printf("removed %lld documents %lld\n", n, (long long)index.num_documents());
    print_rows("after", index.search_batch(qs.data(), nq, p, /*parallel=*/true));
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  return 0;
}
