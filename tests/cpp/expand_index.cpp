// The C++ mirror's expand on a real device (tests/test_gpu_index_expand.py builds it against libnextplaid_hip.so):
//   expand_index <index_dir> <work_dir>
// loads the directory and runs update_resident with the documents of <work_dir>/emb.bin + emb_lens.bin (buffer_size 5: the
// expansion mode, centroids are added) -- the handle then equals a second load of the directory, in its counts and in a
// search -- and then expand_arrays with <work_dir>/cen.bin, lens.bin, codes.bin, res.bin on the handle alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "next_plaid.hpp"

namespace {
int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

template <class T>
std::vector<T> read_all(const std::string& path) {
  std::vector<T> v;
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "cannot read %s\n", path.c_str());
    std::exit(2);
  }
  T x;
  while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
  std::fclose(f);
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s index_dir work_dir\n", argv[0]);
    return 2;
  }
  try {
    auto index = next_plaid::MmapIndex::load(argv[1]);
    const std::string work = argv[2];
    const size_t n = index.num_documents(), K = index.num_partitions(), dim = index.embedding_dim();

    // update_resident: the directory expands, the handle follows without a reload
    const std::vector<float> emb = read_all<float>(work + "/emb.bin");
    next_plaid::Documents docs;
    docs.embeddings = emb.data();
    docs.doc_lengths = read_all<int64_t>(work + "/emb_lens.bin");
    docs.dim = dim;
    next_plaid::UpdateConfig cfg;
    cfg.start_from_scratch = 0;
    cfg.buffer_size = 5;
    cfg.kmeans_niters = 3;
    cfg.max_points_per_centroid = 16;
    np_update_report rep{};
    const std::vector<int64_t> ids = index.update_resident(docs, cfg, nullptr, &rep);
    const size_t m = docs.doc_lengths.size();
    CHECK(rep.mode == NP_UPDATE_EXPAND && rep.n_new_centroids > 0 && rep.n_reindexed == 0);
    CHECK(ids.size() == m && ids.front() == (int64_t)n && index.num_documents() == n + m);
    CHECK(index.num_partitions() == K + (size_t)rep.n_new_centroids);
    {
      auto fresh = next_plaid::MmapIndex::load(argv[1]);
      CHECK(fresh.num_documents() == index.num_documents() && fresh.num_partitions() == index.num_partitions());
      CHECK(fresh.num_embeddings() == index.num_embeddings() && fresh.avg_doclen() == index.avg_doclen());
      const next_plaid::Query q{emb.data(), (size_t)docs.doc_lengths[0]};
      next_plaid::SearchParameters p;
      p.n_full_scores = 128;
      const auto a = index.search_batch(&q, 1, p, false), b = fresh.search_batch(&q, 1, p, false);
      CHECK(a.size() == 1 && b.size() == 1 && a[0].passage_ids == b[0].passage_ids && a[0].scores == b[0].scores);
      CHECK(!a[0].passage_ids.empty() && a[0].passage_ids[0] == (int64_t)n);
    }

    // expand_arrays on the handle alone: 9 documents, the first 4 replace the tail
    const std::vector<float> cen = read_all<float>(work + "/cen.bin");
    const std::vector<int64_t> lens = read_all<int64_t>(work + "/lens.bin"), codes = read_all<int64_t>(work + "/codes.bin");
    const std::vector<uint8_t> res = read_all<uint8_t>(work + "/res.bin");
    const size_t k_new = cen.size() / dim, n1 = index.num_documents(), K1 = index.num_partitions();
    const std::vector<int64_t> got = index.expand_arrays(cen.data(), (int64_t)k_new, lens, codes.data(), res.data(), 4);
    CHECK(got.size() == lens.size() && got.front() == (int64_t)n1 - 4 && index.num_documents() == n1 - 4 + lens.size());
    CHECK(index.num_partitions() == K1 + k_new);

    // refused by name, the handle as it was
    try {
      (void)index.expand_arrays(cen.data(), (int64_t)k_new, lens, codes.data(), res.data(), (int64_t)lens.size() + 1);
      CHECK(!"n_replace beyond n_docs was accepted");
    } catch (const next_plaid::Error& e) {
      CHECK(std::string(e.what()).find("np_hip_index_expand: n_replace is 10") != std::string::npos);
    }
    CHECK(index.num_partitions() == K1 + k_new && index.num_documents() == n1 - 4 + lens.size());
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
