// Text predicates through next_plaid.hpp on an index directory:
//   text_match <index_dir> <codes.i32> <valid.u8> <z.i64> <text.bytes> <offsets.i64> <dfa0.u32> <dfa1.u32>
// Column 0 is the CODE column (codes, validity) whose dictionary is text.bytes / offsets.i64, column 1 the I64 column z; the two
// files dfa*.u32 hold packed DFAs.  Prints
//   match <dfa> <one 0/1 per dictionary string>
// for np_hip_text_match of both DFAs in one call, then
//   ids <filter> <count> <id>...
// for the filters  MATCH(0, dfa0);  NOT MATCH(0, dfa1);  MATCH(0, dfa0) AND z < 2;  MATCH(0, dfa0) OR MATCH(0, dfa1).
// tests/test_gpu_match.py compares the lines with the Python calls.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
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
  if (argc != 9) {
    std::fprintf(stderr, "usage: %s index_dir codes.i32 valid.u8 z.i64 text.bytes offsets.i64 dfa0.u32 dfa1.u32\n", argv[0]);
    return 2;
  }
  try {
    using namespace next_plaid;
    MmapIndex ix = MmapIndex::load(argv[1]);
    const std::vector<int32_t> codes = read_all<int32_t>(argv[2]);
    const std::vector<uint8_t> valid = read_all<uint8_t>(argv[3]);
    const std::vector<int64_t> z = read_all<int64_t>(argv[4]);
    const std::vector<char> text = read_all<char>(argv[5]);
    const std::vector<int64_t> off = read_all<int64_t>(argv[6]);
    const Dfa d0(read_all<uint32_t>(argv[7])), d1(read_all<uint32_t>(argv[8]));
    ix.set_columns({ColumnSpan::codes(codes.data(), codes.size(), valid.data()), ColumnSpan::i64(z.data(), z.size())});
    std::vector<std::string> dictionary;
    for (size_t i = 0; i + 1 < off.size(); ++i) dictionary.emplace_back(text.data() + off[i], (size_t)(off[i + 1] - off[i]));
    ix.set_column_text(0, dictionary);
    np_match_report rep;
    const auto hit = ix.text_match(0, {d0, d1}, dictionary.size(), &rep);
    for (size_t d = 0; d < hit.size(); ++d) {
      std::printf("match %zu ", d);
      for (bool b : hit[d]) std::printf("%d", b ? 1 : 0);
      std::printf("\n");
    }
    std::vector<FilterProgram> f(4);
    f[0].match(0, d0);
    f[1].match(0, d1).not_();
    f[2].match(0, d0).cmp(1, FilterProgram::LT, (int64_t)2).and_();
    f[3].match(0, d0).match(0, d1).or_();
    const auto ids = ix.filter_ids(f);
    for (size_t j = 0; j < ids.size(); ++j) {
      std::printf("ids %zu %zu", j, ids[j].size());
      for (int64_t id : ids[j]) std::printf(" %lld", (long long)id);
      std::printf("\n");
    }
    return rep.tile_bytes > 0 && rep.n_lds + rep.n_global == 2 ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "text_match: %s\n", e.what());
    return 1;
  }
}
