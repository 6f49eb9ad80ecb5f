// Creates an index through next_plaid.hpp (MmapIndex::create_with_kmeans) from raw files:
//   create_index <emb.f32> <lens.i64> <dim> <nbits> <batch_size> <seed> <out_dir>
// tests/test_gpu_index_create.py compares the directory with the one the Python mirror creates.
#include <cstdio>
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
  if (argc != 8) {
    std::fprintf(stderr, "usage: %s emb.f32 lens.i64 dim nbits batch_size seed out_dir\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<float> emb = read_all<float>(argv[1]);
    next_plaid::Documents docs;
    docs.embeddings = emb.data();
    docs.doc_lengths = read_all<int64_t>(argv[2]);
    docs.dim = (size_t)std::atoi(argv[3]);
    next_plaid::IndexConfig cfg;
    cfg.nbits = std::atoi(argv[4]);
    cfg.batch_size = std::atoll(argv[5]);
    cfg.seed = std::strtoull(argv[6], nullptr, 10);
    next_plaid::MmapIndex ix = next_plaid::MmapIndex::create_with_kmeans(docs, argv[7], cfg);
    std::printf("%zu documents\n", (size_t)ix.num_documents());
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
