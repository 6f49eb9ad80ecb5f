// search_exact_grouped through next_plaid.hpp, two ways.
//   search_exact_grouped <index_dir> <queries.f32> <lens.i64> <groups.i32>   (linked with the library; token rows concatenated,
//     their lengths, one dense group id per document): query i is scoped to the even ids below 60 when i is odd.  Prints per query
//     "exact <query> <groups>" and per group " | <group id> <total>" and " <id>:<score bits, hex>" per member: the top 3 groups
//     of 2 at precision 0.  tests/test_gpu_exact_grouped.py compares the lines with the Python call.
//   -DNP_STUBS, no arguments, no library, -fsanitize=address,undefined: the entries the header reaches are recording stubs here;
//     checks the entry's argument values and the slicing of the padded rows (tests/test_exact_grouped_cpu.py).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../next-plaid_amd/cpp/next_plaid.hpp"

using namespace next_plaid;
using Subsets = std::vector<const std::vector<int64_t>*>;

#ifdef NP_STUBS
static struct {
  int B, dim, top_k, gs, precision;
  int64_t n_sub;
  std::vector<float> flat;
  std::vector<int32_t> off, qmap;
  std::vector<int64_t> sid, soff;
} rec;
extern "C" {
const char* np_hip_last_error(void) { return "the stub said so"; }
int np_hip_abi_version(void) { return NP_ABI_VERSION; }
int64_t np_hip_struct_size(int32_t which) { return which == 0 ? (int64_t)sizeof(np_info) : (int64_t)sizeof(np_stats); }
int np_hip_index_open(const char*, const np_open_opts*, np_index** out) {
  static int h;
  *out = reinterpret_cast<np_index*>(&h);
  return NP_OK;
}
void np_hip_index_close(np_index*) {}
int np_hip_index_info(const np_index*, np_info* out) { out->embedding_dim = 8; out->num_documents = 5000; return NP_OK; }
int np_hip_index_probe_dir(const char*, np_info*) { return NP_ERR_IO; }
// counts top_k, 0, 1 in turn; group j of query i: id 10 i + j, members 2 - j % 2 (capped by gs), total members + j
int np_hip_search_exact_grouped(const np_index*, const float* q, const int32_t* off, int32_t B, int32_t dim, int32_t top_k,
                                int32_t gs, int32_t precision, const int64_t* sid, const int64_t* soff, int64_t n,
                                const int32_t* qmap, int64_t* ids, float* sc, int32_t* grp, int32_t* mem, int32_t* tot, int32_t* cnt,
                                np_stats*) {
  rec = {B, dim, top_k, gs, precision, n, {q, q + (size_t)off[B] * dim}, {off, off + B + 1}, {}, {}, {}};
  if (qmap) rec.qmap.assign(qmap, qmap + B);
  if (soff) rec.soff.assign(soff, soff + n + 1), rec.sid.assign(sid, sid + soff[n]);
  for (int i = 0; i < B; ++i) {
    cnt[i] = i % 3 == 0 ? top_k : i % 3 == 1 ? 0 : 1;
    for (int j = 0; j < cnt[i]; ++j) {
      const size_t at = (size_t)i * top_k + j;
      grp[at] = 10 * i + j, mem[at] = std::min(2 - j % 2, gs), tot[at] = mem[at] + j;
      for (int m = 0; m < gs; ++m) ids[at * gs + m] = 1000 * (i + 1) + 10 * j + m, sc[at * gs + m] = (float)(i + j + m);
    }
  }
  return NP_OK;
}
}
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failed; } } while (0)

int main() {
  int failed = 0;
  std::vector<float> rows(7 * 8);
  for (size_t x = 0; x < rows.size(); ++x) rows[x] = (float)x;
  const std::vector<Query> qs{{rows.data(), 3}, {rows.data() + 24, 1}, {rows.data() + 32, 3}};
  const std::vector<int64_t> shared{4, 2, 9};
  MmapIndex ix = MmapIndex::load("an/index");
  for (int scoped = 0; scoped < 2; ++scoped) {
    const auto res = scoped ? ix.search_exact_grouped(qs.data(), 3, 5, 2, 3, Subsets{&shared, nullptr, &shared})
                            : ix.search_exact_grouped(qs.data(), 3, 5);
    CHECK(rec.B == 3 && rec.dim == 8 && rec.top_k == 5 && rec.gs == (scoped ? 2 : 1) && rec.precision == (scoped ? 3 : 0));
    CHECK(rec.flat == rows && rec.off == (std::vector<int32_t>{0, 3, 4, 7}));
    if (scoped)
      CHECK(rec.n_sub == 1 && rec.sid == shared && rec.soff == (std::vector<int64_t>{0, 3}) && rec.qmap == (std::vector<int32_t>{0, -1, 0}));
    else CHECK(rec.n_sub == 0 && rec.sid.empty());
    CHECK(res.size() == 3 && res[0].size() == 5 && res[1].empty() && res[2].size() == 1);
    for (size_t i = 0; i < res.size(); ++i)
      for (size_t j = 0; j < res[i].size(); ++j) {
        const MmapIndex::Group& g = res[i][j];
        const size_t m = std::min<size_t>(2 - j % 2, rec.gs);
        CHECK(g.group_id == (int32_t)(10 * i + j) && g.total == (int32_t)(m + j) && g.passage_ids.size() == m);
        for (size_t x = 0; x < g.passage_ids.size(); ++x)
          CHECK(g.passage_ids[x] == (int64_t)(1000 * (i + 1) + 10 * j + x) && g.scores[x] == (float)(i + j + x));
      }
  }
  if (!failed) std::printf("all checks passed\n");
  return failed != 0;
}
#else
template <class T>
static std::vector<T> read_all(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  std::vector<T> v(b.size() / sizeof(T));
  std::memcpy(v.data(), b.data(), v.size() * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  if (argc != 5) return 2;
  try {
    MmapIndex ix = MmapIndex::load(argv[1]);
    const std::vector<float> rows = read_all<float>(argv[2]);
    const std::vector<int64_t> lens = read_all<int64_t>(argv[3]);
    const std::vector<int32_t> groups = read_all<int32_t>(argv[4]);
    int32_t n_groups = 0;
    for (int32_t g : groups) n_groups = std::max(n_groups, g + 1);
    ix.set_groups(groups, n_groups);
    std::vector<Query> qs;
    std::vector<int64_t> evens;
    for (int64_t d = 0; d < 60; d += 2) evens.push_back(d);
    Subsets subsets;
    for (size_t i = 0, at = 0; i < lens.size(); at += (size_t)lens[i++]) {
      qs.push_back({rows.data() + at * ix.embedding_dim(), (size_t)lens[i]});
      subsets.push_back(i % 2 == 1 ? &evens : nullptr);
    }
    const auto res = ix.search_exact_grouped(qs.data(), qs.size(), 3, 2, 0, subsets);
    for (size_t i = 0; i < res.size(); ++i) {
      std::printf("exact %zu %zu", i, res[i].size());
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
  } catch (const Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
#endif
