// np_update.cpp -- MmapIndex::update / update_append / delete on the crate's index directory.
//
// Host code: the mode choice (index.rs:1431-1590), update_index (update.rs:771-1120), delete_from_index (delete.rs:43-398),
// the buffer and embeddings files (update.rs:110-370) and the posting-list merge.  The device work -- the outlier search,
// k-means of the outliers and the encoding with the residual norms -- is np_build.hip's and runs before the first file of
// the directory is written.  Rules and divergences: include/nextplaid_hip.h.
#include "np_internal.h"

#include <math.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

namespace np {
namespace {

bool file_exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

std::string cpath(const std::string& dir, int64_t c, const char* suffix) {
  return dir + "/" + std::to_string((long long)c) + suffix;
}
std::string doclens_path(const std::string& dir, int64_t c) {
  return dir + "/doclens." + std::to_string((long long)c) + ".json";
}

// ---- files ------------------------------------------------------------------------------------------------------------
struct Meta {   // metadata.json (index.rs:104-155)
  int64_t num_chunks = 0, nbits = 0, num_partitions = 0, num_embeddings = 0, num_documents = 0, dim = 0;
  double avg_doclen = 0.0;
  bool compatible = true;
};

int read_ints(const std::string& path, std::vector<int64_t>* out) {
  std::string j;
  NP_TRY(read_text_file(path, &j));
  out->clear();
  return json_int_list(path, j, out);
}

std::string int_list(const int64_t* v, size_t n) {   // serde_json::to_writer of a Vec<i64>
  std::string s = "[";
  for (size_t i = 0; i < n; ++i) {
    if (i) s += ",";
    s += std::to_string((long long)v[i]);
  }
  return s + "]";
}

int read_meta(const std::string& dir, Meta* m) {
  std::string j;
  if (read_text_file(dir + "/metadata.json", &j) != NP_OK) {
    const std::string e = last_error();
    set_error("Index load failed: Failed to open metadata: %s", e.c_str());
    return NP_ERR_INDEX_LOAD;
  }
  double v;
  if (!json_number_field(j, "num_chunks", &v) || !json_number_field(j, "nbits", &v)) {
    set_error("Index load failed: metadata.json lacks num_chunks / nbits");
    return NP_ERR_INDEX_LOAD;
  }
  json_number_field(j, "num_chunks", &v);
  m->num_chunks = (int64_t)v;
  json_number_field(j, "nbits", &v);
  m->nbits = (int64_t)v;
  m->num_partitions = json_number_field(j, "num_partitions", &v) ? (int64_t)v : 0;
  m->num_embeddings = json_number_field(j, "num_embeddings", &v) ? (int64_t)v : 0;
  m->avg_doclen = json_number_field(j, "avg_doclen", &v) ? v : 0.0;
  m->dim = json_number_field(j, "embedding_dim", &v) ? (int64_t)v : 0;
  m->compatible = j.find("\"next_plaid_compatible\": false") == std::string::npos &&
                  j.find("\"next_plaid_compatible\":false") == std::string::npos;
  if (json_number_field(j, "num_documents", &v) && v > 0) {
    m->num_documents = (int64_t)v;
  } else {   // Metadata::load_from_path infers it from the doclens
    m->num_documents = 0;
    std::vector<int64_t> dl;
    for (int64_t c = 0; c < m->num_chunks; ++c) {
      NP_TRY(read_ints(doclens_path(dir, c), &dl));
      m->num_documents += (int64_t)dl.size();
    }
  }
  return NP_OK;
}

int write_meta(const std::string& dir, const Meta& m) {   // the field order of np_hip_index_write_dir / the crate's Metadata
  return write_text_file(dir + "/metadata.json",
                         "{\n  \"num_chunks\": " + std::to_string((long long)m.num_chunks) + ",\n  \"nbits\": " +
                             std::to_string((long long)m.nbits) + ",\n  \"num_partitions\": " +
                             std::to_string((long long)m.num_partitions) + ",\n  \"num_embeddings\": " +
                             std::to_string((long long)m.num_embeddings) + ",\n  \"avg_doclen\": " + format_f64(m.avg_doclen) +
                             ",\n  \"num_documents\": " + std::to_string((long long)m.num_documents) + ",\n  \"embedding_dim\": " +
                             std::to_string((long long)m.dim) + ",\n  \"next_plaid_compatible\": " +
                             (m.compatible ? "true" : "false") + "\n}");
}

struct ChunkMeta {
  int64_t num_documents = -1, num_embeddings = 0, embedding_offset = 0;
  bool has_offset = false;
};

int read_chunk_meta(const std::string& dir, int64_t c, ChunkMeta* cm) {
  std::string j;
  NP_TRY(read_text_file(cpath(dir, c, ".metadata.json"), &j));
  double v;
  cm->num_documents = json_number_field(j, "num_documents", &v) ? (int64_t)v : -1;
  cm->num_embeddings = json_number_field(j, "num_embeddings", &v) ? (int64_t)v : 0;
  cm->has_offset = json_number_field(j, "embedding_offset", &v);
  cm->embedding_offset = cm->has_offset ? (int64_t)v : 0;
  return NP_OK;
}

int write_chunk_meta(const std::string& dir, int64_t c, const ChunkMeta& cm) {
  std::string s = "{\n  \"num_documents\": " + std::to_string((long long)cm.num_documents) + ",\n  \"num_embeddings\": " +
                  std::to_string((long long)cm.num_embeddings);
  if (cm.has_offset) s += ",\n  \"embedding_offset\": " + std::to_string((long long)cm.embedding_offset);
  return write_text_file(cpath(dir, c, ".metadata.json"), s + "\n}");
}

// an NPY array of one of the given dtypes and rank; rows / cols from its shape (cols = 1 for rank 1)
int read_array(const std::string& path, const char* descr_a, const char* descr_b, size_t ndim, std::vector<uint8_t>* bytes,
               const uint8_t** data, int64_t* rows, int64_t* cols, std::string* descr_out = nullptr) {
  std::string descr;
  std::vector<int64_t> shape;
  NP_TRY(read_npy_file(path, bytes, &descr, &shape, data));
  const auto same = [&](const char* d) { return d && (descr == d || (d[0] == '|' && descr.size() == 3 && descr.substr(1) == d + 1)); };
  if (!same(descr_a) && !same(descr_b)) {
    set_error("Unexpected dtype '%s' in %s", descr.c_str(), path.c_str());
    return NP_ERR_INDEX_LOAD;
  }
  if (shape.size() != ndim) {
    set_error("Unexpected rank %zu in %s", shape.size(), path.c_str());
    return NP_ERR_SHAPE;
  }
  *rows = shape[0];
  *cols = ndim == 2 ? shape[1] : 1;
  if (descr_out) *descr_out = descr;
  return NP_OK;
}

template <class T>
int read_vec(const std::string& path, const char* descr, size_t ndim, std::vector<T>* out, int64_t* rows, int64_t* cols) {
  std::vector<uint8_t> b;
  const uint8_t* d;
  NP_TRY(read_array(path, descr, nullptr, ndim, &b, &d, rows, cols));
  out->resize((size_t)(*rows * *cols));
  if (!out->empty()) memcpy(out->data(), d, out->size() * sizeof(T));
  return NP_OK;
}

int read_ivf_lengths(const std::string& path, std::vector<int32_t>* out) {   // <i4, or fast-plaid's <i8
  std::vector<uint8_t> b;
  const uint8_t* d;
  int64_t rows, cols;
  std::string descr;
  NP_TRY(read_array(path, "<i4", "<i8", 1, &b, &d, &rows, &cols, &descr));
  out->resize((size_t)rows);
  for (int64_t i = 0; i < rows; ++i) {
    if (descr == "<i4") {
      memcpy(&(*out)[(size_t)i], d + 4 * i, 4);
    } else {
      int64_t v;
      memcpy(&v, d + 8 * i, 8);
      (*out)[(size_t)i] = (int32_t)v;
    }
  }
  return NP_OK;
}

int write_f32_2d(const std::string& path, const float* x, int64_t rows, int64_t cols) {
  const int64_t s[2] = {rows, cols};
  return write_npy_file(path, "<f4", s, 2, x, (size_t)(rows * cols) * 4);
}
int write_i64_1d(const std::string& path, const int64_t* x, int64_t n) {
  return write_npy_file(path, "<i8", &n, 1, x, (size_t)n * 8);
}
int write_i32_1d(const std::string& path, const int32_t* x, int64_t n) {
  return write_npy_file(path, "<i4", &n, 1, x, (size_t)n * 4);
}
int write_u8_2d(const std::string& path, const uint8_t* x, int64_t rows, int64_t cols) {
  const int64_t s[2] = {rows, cols};
  return write_npy_file(path, "|u1", s, 2, x, (size_t)(rows * cols));
}

void remove_files(const std::string& dir, std::initializer_list<const char*> names) {
  for (const char* n : names) unlink((dir + "/" + n).c_str());
}

void clear_merged(const std::string& dir) {   // mmap.rs:1714-1743
  remove_files(dir, {"merged_codes.npy", "merged_codes.npy.tmp", "merged_codes.manifest.json", "merged_codes.manifest.json.tmp",
                     "merged_residuals.npy", "merged_residuals.npy.tmp", "merged_residuals.manifest.json",
                     "merged_residuals.manifest.json.tmp"});
}

// documents stored flat next to the index (embeddings.npy, buffer.npy; update.rs:110-370)
struct FlatDocs {
  std::vector<float> x;          // [rows][dim]
  std::vector<int64_t> lens;     // documents (rows past the last whole document are dropped, as load_buffer does)
  int64_t dim = 0, rows = 0;
};

// load_embeddings_npy / load_buffer: the lengths file splits the rows; without it the rows are one document
int load_flat(const std::string& npy, const std::string& lengths, bool unreadable_is_empty, FlatDocs* out) {
  *out = FlatDocs();
  if (!file_exists(npy)) return NP_OK;
  int64_t cols = 0;
  const int rc = read_vec(npy, "<f4", 2, &out->x, &out->rows, &cols);
  if (rc != NP_OK) {
    if (unreadable_is_empty) {
      *out = FlatDocs();
      clear_error();
      return NP_OK;
    }
    return rc;
  }
  out->dim = cols;
  if (!file_exists(lengths)) {
    out->lens.push_back(out->rows);
    return NP_OK;
  }
  std::vector<int64_t> l;
  NP_TRY(read_ints(lengths, &l));
  int64_t off = 0;
  for (int64_t n : l) {
    if (n < 0 || off + n > out->rows) break;
    out->lens.push_back(n);
    off += n;
  }
  return NP_OK;
}

int save_flat(const std::string& dir, const char* npy, const char* lengths, const float* x, int64_t rows, int64_t dim,
              const std::vector<int64_t>& lens) {
  NP_TRY(write_f32_2d(dir + "/" + npy, x, rows, dim));
  return write_text_file(dir + "/" + lengths, int_list(lens.data(), lens.size()));
}

// clean_embeddings_files (delete.rs:270-398): the rows of deleted documents leave embeddings.npy and buffer.npy
int clean_flat(const std::string& dir, const char* npy, const char* lengths, const char* info,
               const std::vector<char>& is_del, int64_t first_id_of /* -1: ids from 0; else original_n */) {
  const std::string pn = dir + "/" + npy, pl = dir + "/" + lengths;
  if (!file_exists(pn) || !file_exists(pl)) return NP_OK;
  std::vector<float> x;
  int64_t rows, dim;
  NP_TRY(read_vec(pn, "<f4", 2, &x, &rows, &dim));
  std::vector<int64_t> l;
  NP_TRY(read_ints(pl, &l));
  const int64_t base = first_id_of < 0 ? 0 : first_id_of - (int64_t)l.size();
  std::vector<float> nx;
  std::vector<int64_t> nl;
  int64_t off = 0;
  for (size_t i = 0; i < l.size(); ++i) {
    const int64_t id = base + (int64_t)i;
    if (!(id >= 0 && id < (int64_t)is_del.size() && is_del[(size_t)id])) {
      for (int64_t r = off; r < std::min(rows, off + l[i]); ++r) nx.insert(nx.end(), &x[(size_t)(r * dim)], &x[(size_t)((r + 1) * dim)]);
      nl.push_back(l[i]);
    }
    off += l[i];
  }
  if (nl.empty()) {
    unlink(pn.c_str());
    unlink(pl.c_str());
    if (info) unlink((dir + "/" + info).c_str());
    return NP_OK;
  }
  NP_TRY(save_flat(dir, npy, lengths, nx.data(), (int64_t)nx.size() / std::max<int64_t>(dim, 1), dim, nl));
  if (info) NP_TRY(write_text_file(dir + "/" + info, "{\"num_docs\":" + std::to_string(nl.size()) + "}"));
  return NP_OK;
}

// ---- delete_from_index (delete.rs:43-268) -------------------------------------------------------------------------------
int delete_impl(const std::string& dir, const int64_t* ids, int64_t n_ids, bool clean_buffer, int64_t* out_deleted) {
  Meta m;
  NP_TRY(read_meta(dir, &m));
  const int64_t N = m.num_documents;
  std::vector<char> is_del((size_t)std::max<int64_t>(N, 0), 0);
  for (int64_t i = 0; i < n_ids; ++i)
    if (ids[i] >= 0 && ids[i] < N) is_del[(size_t)ids[i]] = 1;   // the documented divergence: other ids are ignored
  std::vector<int64_t> del;
  for (int64_t d = 0; d < N; ++d)
    if (is_del[(size_t)d]) del.push_back(d);
  int64_t doc0 = 0, final_docs = 0, total_emb = 0, deleted = 0;
  std::vector<int64_t> dl, codes;
  std::vector<uint8_t> res;
  for (int64_t c = 0; c < m.num_chunks; ++c) {
    NP_TRY(read_ints(doclens_path(dir, c), &dl));
    std::vector<int64_t> ndl;
    bool hit = false;
    for (size_t i = 0; i < dl.size(); ++i) {
      const int64_t id = doc0 + (int64_t)i;
      if (id < N && is_del[(size_t)id]) {
        hit = true;
        ++deleted;
      } else {
        ndl.push_back(dl[i]);
      }
    }
    if (hit) {
      int64_t nc, one, nr, pd;
      NP_TRY(read_vec(cpath(dir, c, ".codes.npy"), "<i8", 1, &codes, &nc, &one));
      NP_TRY(read_vec(cpath(dir, c, ".residuals.npy"), "|u1", 2, &res, &nr, &pd));
      std::vector<int64_t> kc;
      std::vector<uint8_t> kr;
      int64_t t = 0;
      for (size_t i = 0; i < dl.size(); ++i) {
        const int64_t id = doc0 + (int64_t)i;
        const bool keep = !(id < N && is_del[(size_t)id]);
        for (int64_t j = 0; j < dl[i]; ++j, ++t)
          if (keep && t < nc && t < nr) {
            kc.push_back(codes[(size_t)t]);
            kr.insert(kr.end(), &res[(size_t)(t * pd)], &res[(size_t)((t + 1) * pd)]);
          }
      }
      NP_TRY(write_text_file(doclens_path(dir, c), int_list(ndl.data(), ndl.size())));
      NP_TRY(write_i64_1d(cpath(dir, c, ".codes.npy"), kc.data(), (int64_t)kc.size()));
      NP_TRY(write_u8_2d(cpath(dir, c, ".residuals.npy"), kr.data(), (int64_t)kc.size(), pd));
      ChunkMeta cm;
      NP_TRY(read_chunk_meta(dir, c, &cm));
      cm.num_documents = (int64_t)ndl.size();
      cm.num_embeddings = (int64_t)kc.size();
      NP_TRY(write_chunk_meta(dir, c, cm));
    }
    final_docs += (int64_t)ndl.size();
    for (int64_t l : ndl) total_emb += l;
    doc0 += (int64_t)dl.size();
  }
  // posting lists: drop the deleted ids, renumber the rest by the count of deleted ids below them
  {
    std::vector<int64_t> ivf;
    std::vector<int32_t> il;
    int64_t rows, one;
    NP_TRY(read_vec(dir + "/ivf.npy", "<i8", 1, &ivf, &rows, &one));
    NP_TRY(read_ivf_lengths(dir + "/ivf_lengths.npy", &il));
    std::vector<int64_t> nivf;
    nivf.reserve(ivf.size());
    size_t off = 0;
    for (int32_t& len : il) {
      const size_t end = std::min(ivf.size(), off + (size_t)std::max(len, 0));
      int32_t kept = 0;
      for (size_t i = off; i < end; ++i) {
        const int64_t id = ivf[i];
        if (id >= 0 && id < N && is_del[(size_t)id]) continue;
        nivf.push_back(id - (int64_t)(std::lower_bound(del.begin(), del.end(), id) - del.begin()));
        ++kept;
      }
      len = kept;
      off = end;
    }
    NP_TRY(write_i64_1d(dir + "/ivf.npy", nivf.data(), (int64_t)nivf.size()));
    NP_TRY(write_i32_1d(dir + "/ivf_lengths.npy", il.data(), (int64_t)il.size()));
  }
  m.num_embeddings = total_emb;
  m.num_documents = final_docs;
  m.avg_doclen = final_docs > 0 ? (double)total_emb / (double)final_docs : 0.0;
  NP_TRY(write_meta(dir, m));
  clear_merged(dir);
  if (clean_buffer) {
    NP_TRY(clean_flat(dir, "embeddings.npy", "embeddings_lengths.json", nullptr, is_del, -1));
    NP_TRY(clean_flat(dir, "buffer.npy", "buffer_lengths.json", "buffer_info.json", is_del, N));
  }
  if (out_deleted) *out_deleted = deleted;
  return NP_OK;
}

// (old * old_n + new * new_n) / (old_n + new_n) in f32, each product rounded (update.rs:405-407)
float weighted_threshold(float old_thr, int64_t old_n, float new_thr, int64_t new_n) {
#pragma clang fp contract(off)
  return (old_thr * (float)old_n + new_thr * (float)new_n) / (float)(old_n + new_n);
}

// ---- update_index (update.rs:771-1120): the new documents, already encoded, into the chunk files, IVF and metadata --------
int update_index_files(const std::string& dir, const int64_t* lens, int64_t n, const int64_t* codes, const uint8_t* packed,
                       int64_t K, int dim, int64_t batch, const float* norms) {
  Meta m;
  NP_TRY(read_meta(dir, &m));
  const int64_t pd = (int64_t)dim * m.nbits / 8;
  int64_t start = m.num_chunks, cur_off = m.num_embeddings;
  bool append = false;
  if (start > 0 && file_exists(cpath(dir, start - 1, ".metadata.json"))) {
    ChunkMeta last;
    NP_TRY(read_chunk_meta(dir, start - 1, &last));
    if (last.num_documents >= 0 && last.num_documents < 2000) {
      start -= 1;
      append = true;
      cur_off = last.has_offset ? last.embedding_offset : m.num_embeddings - last.num_embeddings;
    }
  }
  const int64_t n_new_chunks = (n + batch - 1) / batch;
  int64_t tok = 0, T = 0;
  for (int64_t i = 0; i < n; ++i) T += lens[i];
  for (int64_t i = 0; i < n_new_chunks; ++i) {
    const int64_t c = start + i, d0 = i * batch, d1 = std::min(n, d0 + batch);
    int64_t nt = 0;
    for (int64_t d = d0; d < d1; ++d) nt += lens[d];
    std::vector<int64_t> cl(lens + d0, lens + d1), cc(codes + tok, codes + tok + nt);
    std::vector<uint8_t> cr(packed + tok * pd, packed + (tok + nt) * pd);
    if (i == 0 && append && file_exists(doclens_path(dir, c))) {   // prepend the last chunk's documents
      std::vector<int64_t> odl, oc;
      std::vector<uint8_t> orr;
      int64_t r, one, pcols;
      NP_TRY(read_ints(doclens_path(dir, c), &odl));
      NP_TRY(read_vec(cpath(dir, c, ".codes.npy"), "<i8", 1, &oc, &r, &one));
      NP_TRY(read_vec(cpath(dir, c, ".residuals.npy"), "|u1", 2, &orr, &r, &pcols));
      if (pcols != pd) {
        set_error("Shape error: chunk %lld residuals have %lld columns, expected %lld", (long long)c, (long long)pcols,
                  (long long)pd);
        return NP_ERR_SHAPE;
      }
      cl.insert(cl.begin(), odl.begin(), odl.end());
      cc.insert(cc.begin(), oc.begin(), oc.end());
      cr.insert(cr.begin(), orr.begin(), orr.end());
    }
    NP_TRY(write_i64_1d(cpath(dir, c, ".codes.npy"), cc.data(), (int64_t)cc.size()));
    NP_TRY(write_u8_2d(cpath(dir, c, ".residuals.npy"), cr.data(), (int64_t)cc.size(), pd));
    NP_TRY(write_text_file(doclens_path(dir, c), int_list(cl.data(), cl.size())));
    ChunkMeta cm;
    cm.num_documents = (int64_t)cl.size();
    cm.num_embeddings = (int64_t)cc.size();
    cm.embedding_offset = cur_off;
    cm.has_offset = true;
    NP_TRY(write_chunk_meta(dir, c, cm));
    cur_off += (int64_t)cc.size();
    tok += nt;
  }
  // update_cluster_threshold (update.rs:385-416)
  if (norms && T > 0) {
    std::vector<float> v(norms, norms + T);
    std::sort(v.begin(), v.end());
    const float q = quantile_of_sorted(v, 0.75);
    float thr = q;
    const std::string tp = dir + "/cluster_threshold.npy";
    if (file_exists(tp)) {
      std::vector<float> old;
      int64_t r, one;
      NP_TRY(read_vec(tp, "<f4", 1, &old, &r, &one));
      if (old.empty()) {
        set_error("Index load failed: cluster_threshold.npy is empty");
        return NP_ERR_INDEX_LOAD;
      }
      thr = weighted_threshold(old[0], m.num_embeddings, q, T);
    }
    const int64_t one = 1;
    NP_TRY(write_npy_file(tp, "<f4", &one, 1, &thr, 4));
  }
  // posting lists: each new document's distinct codes, ids ascending inside a code
  {
    std::vector<int64_t> start_of((size_t)K + 1, 0), pairs_code, pairs_id;
    std::vector<int64_t> dc;
    int64_t t = 0;
    for (int64_t d = 0; d < n; ++d) {
      dc.assign(codes + t, codes + t + lens[d]);
      t += lens[d];
      std::sort(dc.begin(), dc.end());
      dc.erase(std::unique(dc.begin(), dc.end()), dc.end());
      for (int64_t c : dc) {
        pairs_code.push_back(c);
        pairs_id.push_back(m.num_documents + d);
        ++start_of[(size_t)c + 1];
      }
    }
    for (int64_t k = 0; k < K; ++k) start_of[(size_t)k + 1] += start_of[(size_t)k];
    std::vector<int64_t> add(pairs_id.size()), fill(start_of.begin(), start_of.end() - 1);
    for (size_t i = 0; i < pairs_id.size(); ++i) add[(size_t)fill[(size_t)pairs_code[i]]++] = pairs_id[i];
    std::vector<int64_t> ivf;
    std::vector<int32_t> il;
    int64_t rows, one;
    if (file_exists(dir + "/ivf.npy")) NP_TRY(read_vec(dir + "/ivf.npy", "<i8", 1, &ivf, &rows, &one));
    if (file_exists(dir + "/ivf_lengths.npy")) NP_TRY(read_ivf_lengths(dir + "/ivf_lengths.npy", &il));
    std::vector<int64_t> nivf;
    nivf.reserve(ivf.size() + add.size());
    std::vector<int32_t> nil((size_t)K, 0);
    int64_t off = 0;
    std::vector<int64_t> tmp;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t len = k < (int64_t)il.size() ? std::max<int64_t>(il[(size_t)k], 0) : 0;
      const int64_t* old = nullptr;
      int64_t ol = 0;
      if (len > 0 && off + len <= (int64_t)ivf.size()) {
        old = ivf.data() + off;
        ol = len;
      }
      off += len;
      const int64_t* nw = add.data() + start_of[(size_t)k];
      const int64_t nl = start_of[(size_t)k + 1] - start_of[(size_t)k];
      bool asc = true;
      for (int64_t i = 1; i < ol && asc; ++i) asc = old[i - 1] < old[i];
      if (asc && ol > 0 && nl > 0) asc = old[ol - 1] < nw[0];
      const size_t b = nivf.size();
      if (asc) {   // every list this library writes: the new ids are larger, so appending keeps it sorted and unique
        nivf.insert(nivf.end(), old, old + ol);
        nivf.insert(nivf.end(), nw, nw + nl);
      } else {     // any other list: sort and deduplicate with its new entries, as the crate does
        tmp.assign(old, old + ol);
        tmp.insert(tmp.end(), nw, nw + nl);
        std::sort(tmp.begin(), tmp.end());
        tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
        nivf.insert(nivf.end(), tmp.begin(), tmp.end());
      }
      nil[(size_t)k] = (int32_t)(nivf.size() - b);
    }
    NP_TRY(write_i64_1d(dir + "/ivf.npy", nivf.data(), (int64_t)nivf.size()));
    NP_TRY(write_i32_1d(dir + "/ivf_lengths.npy", nil.data(), K));
  }
  Meta nm = m;
  const int64_t total = m.num_documents + n;
  nm.num_chunks = start + n_new_chunks;
  nm.num_partitions = K;
  nm.num_embeddings = m.num_embeddings + T;
  nm.avg_doclen = total > 0 ? (m.avg_doclen * (double)m.num_documents + (double)T) / (double)total : 0.0;
  nm.num_documents = total;
  nm.dim = dim;
  nm.compatible = true;
  NP_TRY(write_meta(dir, nm));
  clear_merged(dir);
  return NP_OK;
}

np_update_config update_defaults(const np_update_config* c) {   // UpdateConfig::default (update.rs:95-107)
  np_update_config o{};
  if (c) o = *c;
  if (o.batch_size == 0) o.batch_size = 50000;
  if (o.kmeans_niters == 0) o.kmeans_niters = 4;
  if (o.max_points_per_centroid == 0) o.max_points_per_centroid = 256;
  if (!c) o.seed = 42;
  if (o.start_from_scratch == 0) o.start_from_scratch = 999;
  if (o.buffer_size == 0) o.buffer_size = 100;
  if (o.buffer_size < 0) o.buffer_size = 0;
  return o;
}

np_index_config kmeans_config(const np_update_config& u, int nbits) {   // index.rs:1472-1483 / update.rs:700-716
  np_index_config c{};
  c.nbits = nbits;
  c.kmeans_niters = u.kmeans_niters;
  c.batch_size = u.batch_size;
  c.seed = u.seed;
  c.max_points_per_centroid = u.max_points_per_centroid;
  c.n_samples_kmeans = u.n_samples_kmeans;
  c.start_from_scratch = u.start_from_scratch;
  return c;
}

struct Codec {
  std::vector<float> centroids, weights, cutoffs;
  int64_t K = 0;
  int dim = 0;
};

int read_codec(const std::string& dir, int nbits, Codec* c) {
  int64_t r, cols;
  NP_TRY(read_vec(dir + "/centroids.npy", "<f4", 2, &c->centroids, &c->K, &cols));
  c->dim = (int)cols;
  NP_TRY(read_vec(dir + "/bucket_weights.npy", "<f4", 1, &c->weights, &r, &cols));
  if (!file_exists(dir + "/bucket_cutoffs.npy")) {
    set_error("Codec error: bucket_cutoffs.npy is required to encode new documents");
    return NP_ERR_CODEC;
  }
  NP_TRY(read_vec(dir + "/bucket_cutoffs.npy", "<f4", 1, &c->cutoffs, &r, &cols));
  if ((int64_t)c->weights.size() != ((int64_t)1 << nbits) || (int64_t)c->cutoffs.size() != ((int64_t)1 << nbits) - 1) {
    set_error("Codec error: bucket tables do not match nbits %d", nbits);
    return NP_ERR_CODEC;
  }
  return NP_OK;
}

// MmapIndex::update (append_only = false) and MmapIndex::update_append (true)
int update_impl(const char* index_dir, const float* emb, const int64_t* lens, int64_t n, int dim,
                const np_update_config* cfg_in, int device, bool append_only, np_update_report* rep) {
  np_update_report R{};
  if (rep) *rep = R;
  if (!index_dir || n < 0 || (n > 0 && !lens)) {
    set_error("index update: invalid argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  const std::string dir = index_dir;
  const np_update_config cfg = update_defaults(cfg_in);
  Meta m;
  NP_TRY(read_meta(dir, &m));
  R.first_doc_id = m.num_documents;
  if (n == 0) {
    if (rep) *rep = R;
    return NP_OK;
  }
  int64_t T = 0;
  for (int64_t d = 0; d < n; ++d) {
    if (lens[d] < 0) {
      set_error("index update: negative document length at %lld", (long long)d);
      return NP_ERR_INVALID_ARGUMENT;
    }
    T += lens[d];
  }
  if (T > 0 && !emb) {
    set_error("index update: embeddings are NULL");
    return NP_ERR_INVALID_ARGUMENT;
  }
  Codec codec;
  auto t0 = std::chrono::steady_clock::now();
  NP_TRY(read_codec(dir, (int)m.nbits, &codec));
  if (dim != codec.dim) {
    set_error("Shape error: embedding dim %d does not match index dim %d", dim, codec.dim);
    return NP_ERR_SHAPE;
  }
  NP_TRY(build_check_dim(dim));
  NP_TRY(build_check_finite(emb, T * dim, dim));
  NP_TRY(build_check_device(device));
  const int nbits = (int)m.nbits;
  const int64_t pd = (int64_t)dim * nbits / 8;

  if (append_only) {
    R.mode = NP_UPDATE_APPEND;
    std::vector<int64_t> codes((size_t)std::max<int64_t>(T, 1));
    std::vector<uint8_t> packed((size_t)std::max<int64_t>(T * pd, 1));
    R.ms_files = ms_since(t0);
    auto t1 = std::chrono::steady_clock::now();
    NP_TRY(encode_with_codec(device, codec.centroids.data(), codec.K, dim, nbits, codec.weights.data(), codec.cutoffs.data(),
                             emb, T, codes.data(), packed.data(), nullptr));
    R.ms_encode = ms_since(t1);
    t1 = std::chrono::steady_clock::now();
    NP_TRY(update_index_files(dir, lens, n, codes.data(), packed.data(), codec.K, dim, cfg.batch_size, nullptr));
    R.ms_files += ms_since(t1);
    if (rep) *rep = R;
    return NP_OK;
  }

  // start from scratch (index.rs:1455-1497)
  if (cfg.start_from_scratch >= 0 && m.num_documents <= cfg.start_from_scratch) {
    FlatDocs old;
    NP_TRY(load_flat(dir + "/embeddings.npy", dir + "/embeddings_lengths.json", false, &old));
    if ((int64_t)old.lens.size() == m.num_documents && (old.lens.empty() || old.dim == dim)) {
      int64_t oT = 0;
      for (int64_t l : old.lens) oT += l;
      std::vector<float> all((size_t)(oT + T) * dim);
      if (oT) memcpy(all.data(), old.x.data(), (size_t)(oT * dim) * 4);
      if (T) memcpy(all.data() + oT * dim, emb, (size_t)(T * dim) * 4);
      std::vector<int64_t> al(old.lens);
      al.insert(al.end(), lens, lens + n);
      const np_index_config ic = kmeans_config(cfg, nbits);
      np_open_opts o{};
      o.device = device;
      auto t1 = std::chrono::steady_clock::now();
      NP_TRY(np_hip_index_create(index_dir, all.data(), al.data(), (int64_t)al.size(), dim, &ic, &o, nullptr));
      if ((int64_t)al.size() > cfg.start_from_scratch) remove_files(dir, {"embeddings.npy", "embeddings_lengths.json"});
      R.mode = NP_UPDATE_SCRATCH;
      R.ms_files = ms_since(t1);
      if (rep) *rep = R;
      return NP_OK;
    }
    // embeddings.npy out of sync (a delete above the threshold): buffer mode
  }

  FlatDocs buf;
  NP_TRY(load_flat(dir + "/buffer.npy", dir + "/buffer_lengths.json", true, &buf));
  if (!buf.lens.empty() && buf.dim != dim) {
    set_error("Shape error: buffer.npy has dim %lld, the index %d", (long long)buf.dim, dim);
    return NP_ERR_SHAPE;
  }
  int64_t bT = 0;
  for (int64_t l : buf.lens) bT += l;
  const int64_t buffer_len = (int64_t)buf.lens.size();
  R.ms_files = ms_since(t0);

  if (n + buffer_len < cfg.buffer_size) {   // buffer mode
    R.mode = NP_UPDATE_BUFFER;
    std::vector<int64_t> codes((size_t)std::max<int64_t>(T, 1));
    std::vector<uint8_t> packed((size_t)std::max<int64_t>(T * pd, 1));
    auto t1 = std::chrono::steady_clock::now();
    NP_TRY(encode_with_codec(device, codec.centroids.data(), codec.K, dim, nbits, codec.weights.data(), codec.cutoffs.data(),
                             emb, T, codes.data(), packed.data(), nullptr));
    R.ms_encode = ms_since(t1);
    t1 = std::chrono::steady_clock::now();
    std::vector<float> all((size_t)std::max<int64_t>((bT + T) * dim, 1));
    if (bT) memcpy(all.data(), buf.x.data(), (size_t)(bT * dim) * 4);
    if (T) memcpy(all.data() + bT * dim, emb, (size_t)(T * dim) * 4);
    std::vector<int64_t> al(buf.lens);
    al.insert(al.end(), lens, lens + n);
    NP_TRY(save_flat(dir, "buffer.npy", "buffer_lengths.json", all.data(), bT + T, dim, al));
    NP_TRY(write_text_file(dir + "/buffer_info.json", "{\"num_docs\":" + std::to_string(al.size()) + "}"));
    NP_TRY(update_index_files(dir, lens, n, codes.data(), packed.data(), codec.K, dim, cfg.batch_size, nullptr));
    R.ms_files += ms_since(t1);
    if (rep) *rep = R;
    return NP_OK;
  }

  // expansion mode (index.rs:1515-1562)
  R.mode = NP_UPDATE_EXPAND;
  int64_t num_buffered = 0;
  {
    std::string j;
    double v;
    if (file_exists(dir + "/buffer_info.json") && read_text_file(dir + "/buffer_info.json", &j) == NP_OK &&
        json_number_field(j, "num_docs", &v) && v > 0)
      num_buffered = (int64_t)v;
    clear_error();
  }
  const bool del_tail = num_buffered > 0 && m.num_documents >= num_buffered;
  R.first_doc_id = (del_tail ? m.num_documents - num_buffered : m.num_documents) + buffer_len;
  R.n_reindexed = buffer_len;
  const int64_t cT = bT + T, cn = buffer_len + n;
  std::vector<float> comb((size_t)std::max<int64_t>(cT * dim, 1));
  if (bT) memcpy(comb.data(), buf.x.data(), (size_t)(bT * dim) * 4);
  if (T) memcpy(comb.data() + bT * dim, emb, (size_t)(T * dim) * 4);
  std::vector<int64_t> cl(buf.lens);
  cl.insert(cl.end(), lens, lens + n);
  NP_TRY(build_check_finite(comb.data(), bT * dim, dim));
  // device work: outliers -> k-means -> encode with the expanded codec + residual norms
  const std::string tp = dir + "/cluster_threshold.npy";
  if (file_exists(tp) && cT > 0) {
    std::vector<float> thr;
    int64_t r, one;
    NP_TRY(read_vec(tp, "<f4", 1, &thr, &r, &one));
    if (thr.empty()) {
      set_error("Index load failed: cluster_threshold.npy is empty");
      return NP_ERR_INDEX_LOAD;
    }
    auto t1 = std::chrono::steady_clock::now();
    std::vector<int64_t> out;
    NP_TRY(find_outliers(device, comb.data(), cT, dim, codec.centroids.data(), codec.K, thr[0], &out, &R.n_rechecked));
    R.ms_outliers = ms_since(t1);
    R.n_outliers = (int64_t)out.size();
    if (!out.empty()) {
      t1 = std::chrono::steady_clock::now();
      const int64_t no = (int64_t)out.size();
      std::vector<float> pts((size_t)no * dim);
      for (int64_t i = 0; i < no; ++i) memcpy(&pts[(size_t)(i * dim)], &comb[(size_t)(out[(size_t)i] * dim)], (size_t)dim * 4);
      const int64_t target =
          std::max<int64_t>(1, (int64_t)ceil((double)no / (double)cfg.max_points_per_centroid)) * 4;   // update.rs:689-693
      const int64_t k_update = std::min(target, no);
      std::vector<float> nc;
      NP_TRY(kmeans_points_as_docs(device, pts.data(), no, dim, kmeans_config(cfg, nbits), k_update, &nc));
      R.n_new_centroids = (int64_t)nc.size() / dim;
      codec.centroids.insert(codec.centroids.end(), nc.begin(), nc.end());
      codec.K += R.n_new_centroids;
      R.ms_kmeans = ms_since(t1);
    }
  }
  std::vector<int64_t> codes((size_t)std::max<int64_t>(cT, 1));
  std::vector<uint8_t> packed((size_t)std::max<int64_t>(cT * pd, 1));
  std::vector<float> norms((size_t)std::max<int64_t>(cT, 1));
  auto t1 = std::chrono::steady_clock::now();
  NP_TRY(encode_with_codec(device, codec.centroids.data(), codec.K, dim, nbits, codec.weights.data(), codec.cutoffs.data(),
                           comb.data(), cT, codes.data(), packed.data(), norms.data()));
  R.ms_encode = ms_since(t1);
  // files
  t1 = std::chrono::steady_clock::now();
  if (del_tail) {
    std::vector<int64_t> tail;
    for (int64_t d = m.num_documents - num_buffered; d < m.num_documents; ++d) tail.push_back(d);
    int64_t gone = 0;
    NP_TRY(delete_impl(dir, tail.data(), (int64_t)tail.size(), false, &gone));   // delete_from_index_keep_buffer
  }
  if (R.n_new_centroids > 0) NP_TRY(write_f32_2d(dir + "/centroids.npy", codec.centroids.data(), codec.K, dim));
  remove_files(dir, {"buffer.npy", "buffer_lengths.json", "buffer_info.json"});   // clear_buffer
  NP_TRY(update_index_files(dir, cl.data(), cn, codes.data(), packed.data(), codec.K, dim, cfg.batch_size, norms.data()));
  R.ms_files += ms_since(t1);
  if (rep) *rep = R;
  return NP_OK;
}

}  // namespace
}  // namespace np

using namespace np;

extern "C" {

int np_hip_index_update(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                        int32_t dim, const np_update_config* cfg, int32_t device, np_update_report* report) {
  clear_error();
  return update_impl(index_dir, embeddings, doc_lengths, n_docs, dim, cfg, device, false, report);
}

int np_hip_index_update_append(const char* index_dir, const float* embeddings, const int64_t* doc_lengths, int64_t n_docs,
                               int32_t dim, const np_update_config* cfg, int32_t device, np_update_report* report) {
  clear_error();
  return update_impl(index_dir, embeddings, doc_lengths, n_docs, dim, cfg, device, true, report);
}

int np_hip_index_delete(const char* index_dir, const int64_t* doc_ids, int64_t n_ids, int64_t* out_deleted) {
  clear_error();
  if (out_deleted) *out_deleted = 0;
  if (!index_dir || n_ids < 0 || (n_ids > 0 && !doc_ids)) {
    set_error("index delete: invalid argument");
    return NP_ERR_INVALID_ARGUMENT;
  }
  return delete_impl(index_dir, doc_ids, n_ids, true, out_deleted);
}

}  // extern "C"
