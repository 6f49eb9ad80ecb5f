// The C++ mirror's keeping remove and append with rows on a real device (tests/test_gpu_index_attach.py builds it against
// libnextplaid_hip.so):
//   attach_index <index_dir> <work_dir> <residual_row_bytes>
// loads the directory, attaches three columns and groups, remove_ids(..., keep_attachments) and append_arrays(..., rows) -- the
// tokens of <work_dir>/lens.bin, codes.bin, res.bin -- and compares get_column / get_groups with the rows worked out here.
#include <cmath>
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
template <class T>
bool same_bytes(const std::vector<uint8_t>& got, const std::vector<T>& want) {
  return got.size() == want.size() * sizeof(T) && (want.empty() || std::memcmp(got.data(), want.data(), got.size()) == 0);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s index_dir work_dir residual_row_bytes\n", argv[0]);
    return 2;
  }
  try {
    auto index = next_plaid::MmapIndex::load(argv[1]);
    const std::string work = argv[2];
    const size_t n = (size_t)index.num_documents();
    std::vector<int64_t> a(n);
    std::vector<uint8_t> av(n);
    std::vector<int32_t> c(n), g(n);
    std::vector<double> x(n);
    for (size_t d = 0; d < n; ++d) {
      a[d] = 3 * (int64_t)d, av[d] = d % 5 != 0, c[d] = (int32_t)(d % 4), g[d] = (int32_t)(d % 6);
      x[d] = d == 7 ? std::nan("") : 0.5 * (double)d;
    }
    index.set_columns({next_plaid::ColumnSpan::i64(a.data(), n, av.data()), next_plaid::ColumnSpan::codes(c.data(), n),
                       next_plaid::ColumnSpan::f64(x.data(), n)});
    index.set_groups(g, 6);
    CHECK(index.get_column(2).has_valid && !index.get_column(1).has_valid);

    // the keeping remove: ids outside the index are ignored, duplicates count once
    const std::vector<int64_t> gone = {1, 7, 64, 7, (int64_t)n - 1, (int64_t)n, -3};
    CHECK(index.remove_ids(gone, /*keep_attachments=*/true) == 4);
    std::vector<int64_t> a1;
    std::vector<uint8_t> av1;
    std::vector<int32_t> c1, g1;
    std::vector<double> x1;
    for (size_t d = 0; d < n; ++d)
      if (d != 1 && d != 7 && d != 64 && d != n - 1) a1.push_back(a[d]), av1.push_back(av[d]), c1.push_back(c[d]), g1.push_back(g[d]), x1.push_back(x[d]);
    CHECK((size_t)index.num_documents() == n - 4);
    auto col = index.get_column(0);
    CHECK(col.type == NP_COL_I64 && col.has_valid && same_bytes(col.data, a1) && col.valid == av1);
    col = index.get_column(1);
    CHECK(col.type == NP_COL_CODE && !col.has_valid && same_bytes(col.data, c1));
    col = index.get_column(2);
    CHECK(col.type == NP_COL_F64 && !col.has_valid && same_bytes(col.data, x1));   // the only NULL row left: no bitmap
    CHECK(index.get_groups() == g1);

    // the append with rows: a remap that shifts every old code by one, a first NULL for the f64 column, a new group
    const std::vector<int64_t> lens = read_all<int64_t>(work + "/lens.bin"), codes = read_all<int64_t>(work + "/codes.bin");
    const std::vector<uint8_t> res = read_all<uint8_t>(work + "/res.bin");
    const size_t m = lens.size();
    std::vector<int64_t> a2(m);
    std::vector<int32_t> c2(m), g2(m);
    std::vector<double> x2(m);
    for (size_t d = 0; d < m; ++d) a2[d] = 1000 + (int64_t)d, c2[d] = (int32_t)((d * 3) % 5), g2[d] = (int32_t)((d * 5) % 7), x2[d] = d == 1 ? std::nan("") : -1.0 * (double)d;
    const std::vector<int32_t> remap = {1, 2, 3, 4};
    next_plaid::MmapIndex::AppendedRows rows;
    rows.columns = {next_plaid::ColumnSpan::i64(a2.data(), m), next_plaid::ColumnSpan::codes(c2.data(), m), next_plaid::ColumnSpan::f64(x2.data(), m)};
    rows.code_remap = {nullptr, remap.data(), nullptr};
    rows.groups = g2;
    rows.n_groups = 7;
    const std::vector<int64_t> ids = index.append_arrays(lens, codes.data(), res.data(), rows);
    CHECK(ids.size() == m && ids.front() == (int64_t)n - 4 && (size_t)index.num_documents() == n - 4 + m);
    for (int32_t& v : c1) v += 1;
    a1.insert(a1.end(), a2.begin(), a2.end()), c1.insert(c1.end(), c2.begin(), c2.end());
    g1.insert(g1.end(), g2.begin(), g2.end()), x1.insert(x1.end(), x2.begin(), x2.end());
    av1.insert(av1.end(), m, 1);
    std::vector<uint8_t> xv(x1.size(), 1);
    xv[n - 4 + 1] = 0;
    col = index.get_column(0);
    CHECK(col.has_valid && same_bytes(col.data, a1) && col.valid == av1);
    col = index.get_column(1);
    CHECK(!col.has_valid && same_bytes(col.data, c1));
    col = index.get_column(2);
    CHECK(col.has_valid && same_bytes(col.data, x1) && col.valid == xv);
    CHECK(index.get_groups() == g1);

    // refused by name, the handle as it was
    rows.columns.pop_back();
    rows.code_remap.clear();
    try {
      (void)index.append_arrays(lens, codes.data(), res.data(), rows);
      CHECK(!"a wrong column count was accepted");
    } catch (const next_plaid::Error& e) {
      CHECK(std::string(e.what()).find("np_hip_index_append_rows: n_cols is 2, the handle has 3 columns") != std::string::npos);
    }
    CHECK((size_t)index.num_documents() == n - 4 + m && index.get_groups() == g1);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  if (failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
