// pool_host.cpp -- the host yardstick of tools/pool_time.py: the pooling of np_pool.hip (the reference's algorithm: cosine
// distances in f64, Ward linkage by nearest-neighbour chain with its cache, the cut in chain order or by distance, f32 means)
// as plain C++ on `threads` host threads, one document at a time per thread.  Same results, bit for bit; the tool asserts it.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC -pthread (contraction off: no product and sum may be fused).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <numeric>
#include <thread>
#include <vector>

namespace {

struct Scratch {
  std::vector<double> D, nrm, nnd;
  std::vector<double> Z;
  std::vector<int> sz, nn, active, chain, parent, order, lab;
};

int first_obs(const std::vector<double>& Z, int m, int c) {
  while (c >= m) c = (int)Z[(size_t)(c - m) * 4];
  return c;
}

int root(std::vector<int>& p, int i) {
  while (p[i] != i) {
    p[i] = p[p[i]];
    i = p[i];
  }
  return i;
}

// returns the number of output rows
int64_t pool_one(const float* x, int64_t n, int dim, int factor, int prot, int cut, float* out, Scratch& s) {
  const auto copy_through = [&]() {
    std::memcpy(out, x, (size_t)n * dim * 4);
    return n;
  };
  if (factor <= 1 || n <= prot + 1) return copy_through();
  const int m = (int)(n - prot);
  const int k = std::max(m / factor, 1);
  if (k >= m) return copy_through();
  const float* tp = x + (size_t)prot * dim;
  const int tot = 2 * m - 1;
  const double inf = std::numeric_limits<double>::infinity();
  s.D.assign((size_t)tot * tot, inf);
  s.nrm.resize(m);
  for (int i = 0; i < m; ++i) {
    double q = 0.0;
    for (int f = 0; f < dim; ++f) {
      const double v = (double)tp[(size_t)i * dim + f];
      q += v * v;
    }
    s.nrm[i] = std::sqrt(q);
  }
  for (int i = 0; i < m; ++i) {
    s.D[(size_t)i * tot + i] = 0.0;
    for (int j = i + 1; j < m; ++j) {
      double dot = 0.0;
      for (int f = 0; f < dim; ++f) dot += (double)tp[(size_t)i * dim + f] * (double)tp[(size_t)j * dim + f];
      const double cs = (s.nrm[i] > 0.0 && s.nrm[j] > 0.0) ? dot / (s.nrm[i] * s.nrm[j]) : 0.0;
      double d = 1.0 - cs;
      d = d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d);
      s.D[(size_t)i * tot + j] = s.D[(size_t)j * tot + i] = d * d;
    }
  }
  s.sz.assign(tot, 1);
  s.nn.assign(tot, -1);
  s.nnd.assign(tot, inf);
  s.active.resize(m);
  std::iota(s.active.begin(), s.active.end(), 0);
  const auto find = [&](int i, int* nn, double* nd) {
    *nn = -1;
    *nd = inf;
    for (int j : s.active) {
      if (j == i) continue;
      const double d = s.D[(size_t)i * tot + j];
      if (d < *nd) {
        *nd = d;
        *nn = j;
      }
    }
  };
  for (int i = 0; i < m; ++i) find(i, &s.nn[i], &s.nnd[i]);
  s.chain.clear();
  s.Z.assign((size_t)(m - 1) * 4, 0.0);
  int next = m;
  for (int r = 0; r < m - 1; ++r) {
    if (s.chain.empty()) s.chain.push_back(s.active[0]);
    for (;;) {
      const int cur = s.chain.back();
      if (s.nn[cur] < 0) find(cur, &s.nn[cur], &s.nnd[cur]);
      const int c = s.nn[cur];
      const double cd = s.nnd[cur];
      if (s.chain.size() >= 2 && s.chain[s.chain.size() - 2] == c) {
        const int a = s.chain.back();
        s.chain.pop_back();
        const int b = s.chain.back();
        s.chain.pop_back();
        const int na = s.sz[a], nb = s.sz[b];
        double* z = &s.Z[(size_t)r * 4];
        z[0] = std::min(a, b);
        z[1] = std::max(a, b);
        z[2] = std::sqrt(cd);
        z[3] = na + nb;
        s.active.erase(std::remove_if(s.active.begin(), s.active.end(), [&](int v) { return v == a || v == b; }), s.active.end());
        s.sz[next] = na + nb;
        for (int q : s.active) {
          const int nk = s.sz[q];
          const double t1 = (double)(na + nk) * s.D[(size_t)a * tot + q];
          const double t2 = (double)(nb + nk) * s.D[(size_t)b * tot + q];
          const double t3 = (double)nk * cd;
          const double nw = ((t1 + t2) - t3) / (double)(na + nb + nk);
          s.D[(size_t)next * tot + q] = s.D[(size_t)q * tot + next] = nw;
          if (s.nn[q] == a || s.nn[q] == b) s.nn[q] = -1;
        }
        s.active.push_back(next);
        find(next, &s.nn[next], &s.nnd[next]);
        ++next;
        break;
      }
      s.chain.push_back(c);
    }
  }
  // the cut
  s.order.resize(m - 1);
  std::iota(s.order.begin(), s.order.end(), 0);
  if (cut == 1)
    std::stable_sort(s.order.begin(), s.order.end(), [&](int p, int q) { return s.Z[(size_t)p * 4 + 2] < s.Z[(size_t)q * 4 + 2]; });
  s.parent.resize(m);
  std::iota(s.parent.begin(), s.parent.end(), 0);
  for (int e = 0; e < m - k; ++e) {
    const int r = s.order[e];
    const int a = root(s.parent, first_obs(s.Z, m, (int)s.Z[(size_t)r * 4])), b = root(s.parent, first_obs(s.Z, m, (int)s.Z[(size_t)r * 4 + 1]));
    if (a != b) s.parent[std::max(a, b)] = std::min(a, b);
  }
  s.lab.assign(m, -1);
  int nlab = 0;
  std::vector<int>& first = s.order;   // reuse: label of a root
  first.assign(m, -1);
  for (int i = 0; i < m; ++i) {
    const int rt = root(s.parent, i);
    if (first[rt] < 0) first[rt] = nlab++;
    s.lab[i] = first[rt];
  }
  std::memcpy(out, x, (size_t)prot * dim * 4);
  float* o = out + (size_t)prot * dim;
  std::fill(o, o + (size_t)k * dim, 0.f);
  std::vector<int> cnt(k, 0);
  for (int i = 0; i < m; ++i) {
    const int c = s.lab[i];
    if (c >= k) continue;
    for (int f = 0; f < dim; ++f) o[(size_t)c * dim + f] += tp[(size_t)i * dim + f];
    ++cnt[c];
  }
  for (int c = 0; c < k; ++c) {
    const float d = (float)std::max(cnt[c], 1);
    for (int f = 0; f < dim; ++f) o[(size_t)c * dim + f] = o[(size_t)c * dim + f] / d;
  }
  return prot + k;
}

}  // namespace

// in_rows / out_rows: n_docs + 1 prefix offsets (rows) of the documents in emb / out
extern "C" int pool_host(const float* emb, const int64_t* in_rows, const int64_t* out_rows, int64_t n_docs, int dim, int factor,
                         int prot, int cut, int threads, float* out) {
  std::atomic<int64_t> next{0};
  std::atomic<int> bad{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&]() {
      Scratch s;
      for (;;) {
        const int64_t i = next.fetch_add(1);
        if (i >= n_docs) break;
        const int64_t rows = pool_one(emb + in_rows[i] * dim, in_rows[i + 1] - in_rows[i], dim, factor, prot, cut,
                                      out + out_rows[i] * dim, s);
        if (rows != out_rows[i + 1] - out_rows[i]) bad.store(1);
      }
    });
  for (std::thread& t : pool) t.join();
  return bad.load();
}
