// Updates an index and deletes from it through next_plaid.hpp (MmapIndex::update, MmapIndex::delete_documents):
//   update_index <index_dir> <emb.f32> <lens.i64> <dim> <buffer_size> <delete.i64>
// tests/test_gpu_index_update.py compares the directory with the one the Python mirror leaves.
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
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s index_dir emb.f32 lens.i64 dim buffer_size delete.i64\n", argv[0]);
    return 2;
  }
  try {
    const std::vector<float> emb = read_all<float>(argv[2]);
    next_plaid::Documents docs;
    docs.embeddings = emb.data();
    docs.doc_lengths = read_all<int64_t>(argv[3]);
    docs.dim = (size_t)std::atoi(argv[4]);
    next_plaid::UpdateConfig cfg;
    cfg.buffer_size = std::atoll(argv[5]);
    next_plaid::MmapIndex ix = next_plaid::MmapIndex::load(argv[1]);
    const std::vector<int64_t> ids = ix.update(docs, cfg);
    const int64_t gone = ix.delete_documents(read_all<int64_t>(argv[6]));
    std::printf("%zu ids from %lld, %lld deleted\n", ids.size(), ids.empty() ? -1LL : (long long)ids[0], (long long)gone);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
