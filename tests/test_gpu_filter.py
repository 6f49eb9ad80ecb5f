"""Metadata filters on the device: set_columns, np_hip_filter_eval and the filtered searches.  Needs a real MI355X.

The reference for the ids is tests/filter_restate.py (a numpy evaluator that tests/test_filter_restate_cpu.py pins to SQLite
itself); the reference for a filtered search is the subsets call of the same build on the restatement's ids, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api, filters as F
import filter_restate as R

pytestmark = pytest.mark.gpu

BLOCK_DOCS = 16384   # documents per compaction block (NP_FILTER_BLOCK_DOCS: 256 ballot words of 64): 70 001 crosses it 4 times
COUNTS = [1, 63, 64, 65, 4099, 70001]


def P(**kw):
    return npa.SearchParameters(**kw)


def tiny_index(n_docs, **opts):
    """An index of n_docs one-token documents: the filters only need its document count."""
    spec, a = make_arrays(num_docs=n_docs, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    return a, hip_index(a, **opts)


@pytest.fixture(scope="module", params=COUNTS)
def sized(request):
    n = request.param
    rows = R.make_rows(n)
    a, hx = tiny_index(n)
    hx.set_columns(rows)
    yield n, rows, hx
    hx.close()


def shapes(n):
    """Filters by what they select: nothing, everything, only the last document."""
    return [("1=1", []), ("0=1", []), ("z >= ?", [0]), ("z < ?", [0]), ("docno = ?", [n - 1]), ("docno >= ?", [n - 1]),
            ("docno IN (?, ?, ?)", [0, n - 1, n]), ("NOT docno < ?", [n - 1])]


def test_fixed_list_and_random_expressions_equal_the_restatement(sized):
    n, rows, hx = sized
    sch = hx.schema
    assert sch["z"].valid is None and (sch["y"].valid is not None or n < 63)   # columns without and with a validity array
    assert np.isnan(rows["x"]).any() or n < 40                             # an F64 column whose NULLs come only from NaN
    conds = R.fixed_conditions() + R.random_conditions(100)
    progs = [npa.compile_filter(c, p, sch) for c, p in conds]
    got = hx.filter_ids(progs)                                             # 170+ filters in one call
    assert len(got) == len(conds)
    n_sel = 0
    for (c, p), prog, g in zip(conds, progs, got):
        want = R.select(prog, sch)
        assert g.dtype == np.int64 and np.array_equal(g, want), f"n={n} {c} {p}: {g[:8]} ({g.size}) vs {want[:8]} ({want.size})"
        n_sel += 0 < want.size < n
    assert n_sel > 40 or n < 64
    assert np.array_equal(hx.filter_ids(progs, counts_only=True), [g.size for g in got])


def test_filter_shapes_and_33_filters_in_one_call(sized):
    n, rows, hx = sized
    cols = dict(rows)
    cols["docno"] = np.arange(n, dtype=np.int64)
    hx.set_columns(cols)
    try:
        sch = hx.schema
        conds = shapes(n)
        got = hx.filter_ids(conds)
        assert np.array_equal(got[0], np.arange(n)) and got[1].size == 0 and np.array_equal(got[2], np.arange(n)) and got[3].size == 0
        for g in got[4:]:
            assert np.array_equal(g[-1:], [n - 1])
        assert np.array_equal(got[4], [n - 1]) and np.array_equal(got[5], [n - 1]) and np.array_equal(got[7], [n - 1])
        many = [("docno >= ? AND z != ?", [i * n // 33, i % 5]) for i in range(33)]
        got = hx.filter_ids(many)
        assert len(got) == 33
        for (c, p), g in zip(many, got):
            assert np.array_equal(g, R.ids_of(c, p, sch))
        again = hx.filter_ids(many)                                        # the same bits from run to run
        assert all(np.array_equal(a, b) for a, b in zip(got, again))
    finally:
        hx.set_columns(rows)


@pytest.mark.parametrize("budget", [300_000, 2_000_000])
def test_small_workspace_runs_in_chunks_with_the_same_bits(budget):
    """70 001 documents are 5 compaction blocks; a (filter, block) unit of the id-staging pass is 133 132 bytes, of the resident
    pass 2 060: 300 kB holds one or two staged units (one filter, one block at a time) and 2 MB about fourteen (33 filters in
    chunks of filters and blocks).  The ids must not depend on it."""
    n = 70001
    rows = R.make_rows(n)
    a, hx = tiny_index(n, workspace_bytes=budget)
    try:
        hx.set_columns(rows)
        sch = hx.schema
        conds = [c for c in R.random_conditions(33, seed=21)] + [("1=1", []), ("0=1", []), ("z = ?", [4])]
        got = hx.filter_ids(conds)
        for (c, p), g in zip(conds, got):
            assert np.array_equal(g, R.ids_of(c, p, sch)), f"budget {budget}: {c} {p}"
        assert np.array_equal(hx.filter_ids(conds, counts_only=True), [g.size for g in got])   # (chunks of the counting pass)
    finally:
        hx.close()
    a, tight = tiny_index(n, workspace_bytes=100_000)   # holds no chunk: an error, not a failed launch
    try:
        tight.set_columns(rows)
        with pytest.raises(MemoryError, match="workspace budget"):   # NP_ERR_OUT_OF_MEMORY
            tight.filter_ids([("1=1", [])])
        assert tight.filter_ids([]) == []
    finally:
        tight.close()


def test_three_shards_return_their_own_global_ids():
    n = 4099
    rows = R.make_rows(n)
    spec, a = make_arrays(num_docs=n, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    sch = npa.make_schema(rows, n)
    conds = R.fixed_conditions()[:30] + R.random_conditions(20, seed=4) + [("1=1", [])]
    whole = [R.ids_of(c, p, sch) for c, p in conds]
    parts = []
    for r in range(3):
        hx = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"], a["codes"],
                                       a["residuals"], a["nbits"], shard_rank=r, shard_count=3)
        lo, hi = int(hx.info.shard_doc_begin), int(hx.info.shard_doc_end)
        assert (lo, hi) == (n * r // 3, n * (r + 1) // 3)
        hx.set_columns(rows)                                               # whole-index columns: the handle keeps its slice
        got = hx.filter_ids(conds)
        for w, g in zip(whole, got):
            assert np.array_equal(g, w[(w >= lo) & (w < hi)])
        parts.append(got)
        # filters through the search entry points need the whole index
        q = np.zeros((2, 32), np.float32)
        with pytest.raises(ValueError, match="shard"):
            hx.search_batch([q], P(top_k=3, n_full_scores=16, n_ivf_probe=2), filters=[("1=1", [])])
        with pytest.raises(ValueError, match="shard"):
            hx.search_exact([q], 3, filters=[("1=1", [])])
        hx.close()
    for j, w in enumerate(whole):
        assert np.array_equal(np.concatenate([p[j] for p in parts]), w)


# ---- search equivalence ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[128, 64])
def corpus(request):
    dim = request.param
    spec, a = make_arrays(num_docs=3000, num_centroids=256, dim=dim, nbits=4, doc_len_min=8, doc_len_max=30, seed=41 + dim)
    qs, _ = synth.make_queries(spec, 9, n_tokens=16, cen=a["centroids"])
    rows = R.make_rows(3000, seed=dim)
    return a, qs, rows


BATCH = [("y > ? AND s IS NOT NULL", [0]), ("x < ? OR t LIKE ?", [0.5, "%a%"]), None, ("z = ? AND z = ?", [1, 2]), ("1=1", []),
         ("y > ? AND s IS NOT NULL", (0,)), ("w BETWEEN ? AND ?", [-0.5, 1.0]), ("t IN (?, ?, ?)", ["alpha", "Beta", "ca_x"]),
         ("NOT (x > ?)", [0.0])]


def same_bytes(got, want, what):
    assert len(got) == len(want)
    for i, (r, f) in enumerate(zip(got, want)):
        assert r.query_id == f.query_id
        assert r.passage_ids.tobytes() == f.passage_ids.tobytes() and r.scores.tobytes() == f.scores.tobytes(), \
            f"{what} q{i}: {r.passage_ids} {r.scores} vs {f.passage_ids} {f.scores}"


def reference_subsets(sch):
    subs, seen = [], {}
    for f in BATCH:
        if f is None:
            subs.append(None)
            continue
        key = npa.compile_filter(f[0], f[1], sch).key()
        if key not in seen:                       # equal filters share one subset object, as they share one filter
            seen[key] = R.ids_of(f[0], f[1], sch)
        subs.append(seen[key])
    return subs


@pytest.mark.parametrize("variant", ["prec0", "prec1", "max_batch4", "retain_only"])
def test_search_batch_filters_equal_subsets_of_the_restatement(corpus, variant):
    a, qs, rows = corpus
    hx = hip_index(a, **({"max_batch": 4} if variant == "max_batch4" else {}))
    try:
        hx.set_columns(rows)
        subs = reference_subsets(hx.schema)
        assert subs[3].size == 0 and subs[4].size == 3000 and subs[0] is subs[5] and 0 < subs[0].size < 3000
        p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None, precision=1 if variant == "prec1" else 0,
              **({"centroid_batch_size": 100} if variant == "retain_only" else {}))   # 100 < K = 256: candidate retain only
        want = hx.search_batch(qs, p, subsets=subs)
        got = hx.search_batch(qs, p, filters=BATCH)
        same_bytes(got, want, variant)
        assert got[3].passage_ids.size == 0 and got[2].passage_ids.size == 10 and got[4].passage_ids.size == 10
        assert all(np.isin(r.passage_ids, s).all() for r, s in zip(got, subs) if s is not None)
        assert hx.last_stats["n_queries"] == 9 and hx.last_stats["ms_total"] > 0
        one = hx.search(qs[1], p, filter=BATCH[1])
        assert one.query_id == 0 and one.passage_ids.tobytes() == hx.search(qs[1], p, subset=subs[1]).passage_ids.tobytes()
        assert one.scores.tobytes() == hx.search(qs[1], p, subset=subs[1]).scores.tobytes()
        same_bytes(hx.search_batch(qs, p, filters=[None] * 9), hx.search_batch(qs, p), variant + " no filters")
        with pytest.raises(ValueError):
            hx.search_batch(qs, p, filters=BATCH, subsets=subs)
    finally:
        hx.close()


@pytest.mark.parametrize("variant", ["prec0", "prec3", "max_batch4"])
def test_search_exact_filters_equal_subsets_of_the_restatement(corpus, variant):
    a, qs, rows = corpus
    hx = hip_index(a, **({"max_batch": 4} if variant == "max_batch4" else {}))
    try:
        hx.set_columns(rows)
        subs = reference_subsets(hx.schema)
        prec = 3 if variant == "prec3" else 0
        want = hx.search_exact(qs, 10, prec, subsets=subs)
        got = hx.search_exact(qs, 10, prec, filters=BATCH)
        same_bytes(got, want, variant)
        assert got[3].passage_ids.size == 0 and got[4].passage_ids.size == 10
        with pytest.raises(ValueError):
            hx.search_exact(qs, 10, prec, filters=BATCH, subset=subs[0])
    finally:
        hx.close()


# ---- errors and bookkeeping -----------------------------------------------------------------------------------------------

def test_errors_leave_the_handle_usable_and_device_bytes_follow_the_columns(corpus):
    a, qs, rows = corpus
    hx = hip_index(a)
    try:
        p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
        known = hx.search_batch(qs, p)

        def still_fine():
            same_bytes(hx.search_batch(qs, p), known, "after an error")

        bytes0 = int(hx.info.device_bytes)
        with pytest.raises(npa.NextPlaidError, match="unknown column"):                # no schema yet: the compiler answers
            hx.search_batch(qs, p, filters=[("y = ?", [1])] * 9)
        prog = npa.compile_filter("y = ?", [1], npa.make_schema(rows, 3000))
        with pytest.raises(ValueError, match="no columns"):                    # ... and the library, given a program
            hx.search_batch_filtered(qs, p, [prog], np.zeros(9, np.int32))
        with pytest.raises(ValueError, match="no columns"):
            hx.filter_ids([prog])
        still_fine()
        hx.set_columns(rows)
        sch = hx.schema
        grown = int(hx.info.device_bytes) - bytes0
        data_bytes = sum(c.data.nbytes for c in sch.columns.values())
        assert grown >= data_bytes and grown < data_bytes + 3000 * 6 + 64 * 1024, (grown, data_bytes)
        assert hx.filter_ids([prog])[0].size > 0
        for bad in ([0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 0, -2, 0, 0, 0, 0, 0, 0]):
            with pytest.raises(ValueError, match="query_filter"):
                hx.search_batch_filtered(qs, p, [prog], np.array(bad, np.int32))
            with pytest.raises(ValueError, match="query_filter"):
                hx.search_exact_filtered(qs, 10, 0, [prog], np.array(bad, np.int32))
        still_fine()
        # a malformed program: the message names the filter and the op
        broken = F.CompiledFilter([(F.NP_F_CMP, 0, 0, 1, 0), (F.NP_F_AND, -1, 0, 0, 0)], np.array([1], np.int64))
        with pytest.raises(ValueError, match="filter 1, op 1: stack underflow"):
            hx.filter_ids([prog, broken])
        with pytest.raises(ValueError, match="column index out of range"):
            hx.filter_ids([F.CompiledFilter([(F.NP_F_IS_NULL, 6, 0, 0, 0)], np.zeros(0, np.int64))])
        still_fine()
        # ids_capacity too small: the offsets are still filled in full and the message names the needed size
        all_y = npa.compile_filter("y IS NOT NULL", [], sch)
        want = [R.select(prog, sch), R.select(all_y, sch)]
        rc, off, ids = hx.filter_eval_raw([prog, all_y], want[0].size + want[1].size - 1)
        assert rc == 8 and off.tolist() == [0, want[0].size, want[0].size + want[1].size]
        assert str(want[0].size + want[1].size) in api.last_error()
        rc, off, ids = hx.filter_eval_raw([prog, all_y], want[0].size + want[1].size)
        assert rc == 0 and np.array_equal(ids, np.concatenate(want))
        rc, off, _ = hx.filter_eval_raw([prog, all_y], 0, want_ids=False)                # counts only
        assert rc == 0 and off.tolist() == [0, want[0].size, want[0].size + want[1].size]
        still_fine()
        with pytest.raises(npa.ShapeError):
            hx.set_columns({"y": np.arange(2999)})
        assert hx.filter_ids([prog])[0].size == want[0].size                             # the earlier columns are still there
        hx.set_columns({})
        assert hx.schema is None and int(hx.info.device_bytes) == bytes0
        with pytest.raises(ValueError, match="no columns"):
            hx.search_batch_filtered(qs, p, [prog], np.zeros(9, np.int32))
        with pytest.raises(ValueError, match="no columns"):
            hx.search_exact_filtered(qs, 10, 0, [prog], np.zeros(9, np.int32))
        still_fine()
    finally:
        hx.close()


# ---- C++ mirror -----------------------------------------------------------------------------------------------------------

CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "next_plaid.hpp"
// argv: index dir, queries file (n, tokens, dim as i64, then f32 rows), columns file (n as i64, y i64[n], yv u8[n], x f64[n],
// s i32[n]), output file
int main(int argc, char** argv) {
  if (argc < 5) return 2;
  FILE* f = std::fopen(argv[2], "rb");
  int64_t hdr[3];
  if (!f || std::fread(hdr, 8, 3, f) != 3) return 2;
  const size_t n = (size_t)hdr[0], tok = (size_t)hdr[1], dim = (size_t)hdr[2];
  std::vector<float> rows(n * tok * dim);
  if (std::fread(rows.data(), 4, rows.size(), f) != rows.size()) return 2;
  std::fclose(f);
  std::vector<next_plaid::Query> qs;
  for (size_t i = 0; i < n; ++i) qs.push_back({rows.data() + i * tok * dim, tok});
  f = std::fopen(argv[3], "rb");
  int64_t nd;
  if (!f || std::fread(&nd, 8, 1, f) != 1) return 2;
  std::vector<int64_t> y(nd);
  std::vector<uint8_t> yv(nd);
  std::vector<double> x(nd);
  std::vector<int32_t> s(nd);
  if (std::fread(y.data(), 8, nd, f) != (size_t)nd || std::fread(yv.data(), 1, nd, f) != (size_t)nd ||
      std::fread(x.data(), 8, nd, f) != (size_t)nd || std::fread(s.data(), 4, nd, f) != (size_t)nd)
    return 2;
  std::fclose(f);
  try {
    using FP = next_plaid::FilterProgram;
    auto ix = next_plaid::MmapIndex::load(argv[1]);
    ix.set_columns({next_plaid::ColumnSpan::i64(y.data(), y.size(), yv.data()), next_plaid::ColumnSpan::f64(x.data(), x.size()),
                    next_plaid::ColumnSpan::codes(s.data(), s.size())});
    std::vector<FP> filters(3);
    filters[0].cmp(0, FP::GT, (int64_t)0).is_null(2).not_().and_();                       // y > 0 AND s IS NOT NULL
    filters[1].between(1, -1.0, 0.5).in(2, std::vector<int64_t>{1, 3, 4}, true).not_().or_();   // x BETWEEN .. OR s NOT IN (.., NULL)
    filters[2].in(0, std::vector<int64_t>{-1, 7}).constant(FP::UNKNOWN).or_();            // y IN (-1, 7) OR NULL
    auto ids = ix.filter_ids(filters);
    FILE* o = std::fopen(argv[4], "wb");
    for (auto& v : ids) {
      int64_t c = (int64_t)v.size();
      std::fwrite(&c, 8, 1, o);
      std::fwrite(v.data(), 8, v.size(), o);
    }
    next_plaid::SearchParameters p;
    p.n_full_scores = 256;
    p.top_k = 10;
    p.n_ivf_probe = 4;
    p.centroid_score_threshold = std::nullopt;
    std::vector<int32_t> qf(n);
    for (size_t i = 0; i < n; ++i) qf[i] = (int32_t)(i % 4) - 1;
    auto res = ix.search_batch_filtered(qs.data(), n, p, true, filters, qf);
    auto ex = ix.search_exact_filtered(qs.data(), n, 10, 0, filters, qf);
    res.insert(res.end(), ex.begin(), ex.end());
    for (auto& r : res) {
      int64_t c[2] = {(int64_t)r.query_id, (int64_t)r.passage_ids.size()};
      std::fwrite(c, 8, 2, o);
      std::fwrite(r.passage_ids.data(), 8, r.passage_ids.size(), o);
      std::fwrite(r.scores.data(), 4, r.scores.size(), o);
    }
    std::fclose(o);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  return 0;
}
"""


def test_cpp_mirror_gives_the_same_bytes(corpus, tmp_path):
    a, qs, rows = corpus
    dim = a["centroids"].shape[1]
    src = tmp_path / "filter_cli.cpp"
    src.write_text(CPP)
    exe = tmp_path / "filter_cli"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I",
                           os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib_dir, "-lnextplaid_hip",
                           f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), a, chunk_docs=1100)
    cols = {"y": rows["y"], "x": rows["x"], "s": rows["s"]}
    sch = npa.make_schema(cols, 3000)
    with open(tmp_path / "q.bin", "wb") as f:
        f.write(np.array([len(qs), 16, dim], np.int64).tobytes() + np.concatenate(qs, 0).astype(np.float32).tobytes())
    with open(tmp_path / "cols.bin", "wb") as f:
        f.write(np.array([3000], np.int64).tobytes() + sch["y"].data.tobytes() + sch["y"].valid.tobytes() + sch["x"].data.tobytes()
                + sch["s"].data.tobytes())
    subprocess.check_call([str(exe), str(ixdir), str(tmp_path / "q.bin"), str(tmp_path / "cols.bin"), str(tmp_path / "out.bin")], timeout=120)
    # the same three filters through the Python compiler.  The C++ side passes s without a validity array: its NULL rows read as
    # code 0 there, so the Python columns do the same
    cols["s"] = sch["s"].data
    hx = npa.MmapIndex.load(str(ixdir))
    try:
        hx.set_columns(cols)
        conds = [("y > ? AND s IS NOT NULL", [0]), ("x BETWEEN ? AND ? OR s NOT IN (?, ?, ?, ?)", [-1.0, 0.5, 1, 3, 4, None]),
                 ("y IN (?, ?) OR y = ?", [-1, 7, None])]
        want = b""
        ids = hx.filter_ids(conds)
        assert all(i.size > 0 for i in ids[::2])
        for v in ids:
            want += np.array([v.size], np.int64).tobytes() + v.tobytes()
        p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
        fl = [None if i % 4 == 0 else conds[i % 4 - 1] for i in range(len(qs))]
        for r in hx.search_batch(qs, p, filters=fl) + hx.search_exact(qs, 10, 0, filters=fl):
            want += np.array([r.query_id, r.passage_ids.size], np.int64).tobytes() + r.passage_ids.tobytes() + r.scores.tobytes()
        assert open(tmp_path / "out.bin", "rb").read() == want
    finally:
        hx.close()
