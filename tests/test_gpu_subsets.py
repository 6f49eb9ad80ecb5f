"""One subset per query in one batch (np_hip_search_batch_subsets and its device / phase / sharded forms).  Needs a real MI355X.

The reference for BIT equality is the single-subset path of the same build: query i of a batch with subsets[i] must return what
search(queries[i], params, subsets[i]) returns alone (test_search_equals_batch_of_one: a query's result does not depend on its
batch at precision 2).  The reference for SEMANTICS is the CPU oracle (search.rs:350-382, 434-437 dense; 542-545 batched).
"""
import os
import subprocess

import numpy as np
import pytest

from helpers import (ROOT, RTOL_BF16, RTOL_BF16_PLAIN, RTOL_F32, assert_ranking_close, hip_index, make_arrays, oracle_index, synth,
                     to_oracle_params)

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu


def P(**kw):
    return npa.SearchParameters(**kw)


def rtol_of(prec):
    return RTOL_F32 if prec in (0, 2) else (RTOL_BF16 if prec == 1 else RTOL_BF16_PLAIN)


def same_bits(r, f):
    return np.array_equal(r.passage_ids, f.passage_ids) and np.array_equal(r.scores.view(np.uint32), f.scores.view(np.uint32))


def subset_pool(n_docs):
    """The subsets of issue case 1: half of the documents, a handful with ids outside the index, a dense prefix, none."""
    return dict(evens=np.arange(0, n_docs, 2, dtype=np.int64), odd_ids=np.array([5, 17, n_docs - 1, 2 * n_docs, -3], np.int64),
                head=np.arange(100, dtype=np.int64), empty=np.zeros(0, np.int64))


@pytest.fixture(scope="module")
def small():
    # the existing subset test's index (test_subset_filter_and_empty_subset)
    spec, a = make_arrays(num_docs=2000, num_centroids=256, dim=128, nbits=4, doc_len_min=10, doc_len_max=40, seed=31)
    qs, _ = synth.make_queries(spec, 8, n_tokens=16, cen=a["centroids"])
    return spec, a, oracle_index(a), hip_index(a), qs


def check_against_singles(hx, qs, p, subsets, what, bits=True):
    """The batch's results; each compared with the single-subset call of its query and subset."""
    res = hx.search_batch(qs, p, subsets=subsets)
    assert len(res) == len(qs)
    for i, (q, sub, r) in enumerate(zip(qs, subsets, res)):
        f = hx.search(q, p, sub)
        assert r.query_id == i
        if bits:
            assert same_bits(r, f), f"{what} q{i}: batch {r.passage_ids} {r.scores} vs single {f.passage_ids} {f.scores}"
        else:
            assert_ranking_close(r.passage_ids, r.scores, f.passage_ids, f.scores, rtol_of(p.precision), f"{what} q{i} vs single")
    return res


@pytest.mark.parametrize("prec", [2, 0, 1, 3])
def test_one_query_many_subsets(small, prec):
    """Six copies of one query with [evens, None, ids partly outside the index, arange(100), empty, evens again (the same
    object)]: by search.rs:370-382 the effective probe depths in this ONE launch are 8, 4, n_elig (take-all: at most 120 eligible
    centroids against a scaled depth of 1600), 80 and 0."""
    spec, a, ox, hx, qs = small
    pool = subset_pool(2000)
    q = qs[0]
    subsets = [pool["evens"], None, pool["odd_ids"], pool["head"], pool["empty"], pool["evens"]]
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None, precision=prec)
    # the data must tell a per-query mix-up from a correct run: the single-subset traces differ
    traces = [hx.debug_trace(q, p, s) for s in subsets[:5]]
    cell_lists = {tuple(t["cells"].tolist()) for t in traces}
    assert len(cell_lists) >= 3, f"only {len(cell_lists)} different cell lists among the subsets"
    assert traces[4]["cells"].size == 0 and traces[2]["cells"].size <= 120
    res = check_against_singles(hx, [q] * 6, p, subsets, f"prec={prec}", bits=(prec == 2))
    assert same_bits(res[0], res[5])
    assert res[4].passage_ids.size == 0 and res[4].scores.size == 0
    for i, (sub, r, tr) in enumerate(zip(subsets, res, traces + [traces[0]])):
        if sub is not None:
            assert set(r.passage_ids.tolist()) <= set(sub.tolist()), f"q{i}: a result outside its subset"
        if sub is not None and sub.size == 0:
            continue
        o = ox.search(q, to_oracle_params(p), sub, trace=True)
        t = o.trace
        assert np.array_equal(tr["cells"], t.cells) and np.array_equal(tr["cand"], t.cand), f"q{i}: single-subset trace vs oracle"
        assert np.array_equal(tr["approx"].view(np.uint32), t.approx.view(np.uint32)) and np.array_equal(tr["sel"], t.sel), f"q{i}"
        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, rtol_of(prec), f"prec={prec} q{i} vs oracle")


@pytest.mark.parametrize("bisect", [0, 1])
@pytest.mark.parametrize("slices", [0, 1])
def test_many_queries_mixed_across_slices(small, slices, bisect):
    """Eight different queries, subsets from the same pool, max_batch = 3: the batch runs as three passes and a subset is
    referenced from more than one of them; under both S3 mark kernels, bisecting and sweeping."""
    spec, a, ox, _, qs = small
    hx = hip_index(a, max_batch=3)
    hx.tune("s3_slices", slices)
    hx.tune("s3_bisect", bisect)
    pool = subset_pool(2000)
    subsets = [pool["evens"], pool["head"], None, pool["head"], pool["odd_ids"], pool["evens"], pool["empty"], None]
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
    res = check_against_singles(hx, qs, p, subsets, f"slices={slices} bisect={bisect}")
    for i, (q, sub, r) in enumerate(zip(qs, subsets, res)):
        if sub is not None and sub.size == 0:
            assert r.passage_ids.size == 0
            continue
        o = ox.search(q, to_oracle_params(p), sub)
        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, f"slices={slices} bisect={bisect} q{i}")
    # a batch none of whose queries has a subset is the plain batch
    for r, f in zip(hx.search_batch(qs, p, subsets=[None] * 8), hx.search_batch(qs, p)):
        assert same_bits(r, f)
    hx.close()


def test_batched_path_only_retains(small):
    """K > centroid_batch_size (search.rs:542-545): the subset only filters candidates; the cells are the unfiltered ones."""
    spec, a, ox, hx, qs = small
    pool = subset_pool(2000)
    subsets = [pool["evens"], None, pool["head"], pool["odd_ids"], pool["empty"], pool["head"], None, pool["evens"]]
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None, centroid_batch_size=100)
    res = check_against_singles(hx, qs, p, subsets, "batched")
    for i, (q, sub, r) in enumerate(zip(qs, subsets, res)):
        if sub is None or sub.size == 0:
            continue
        assert np.array_equal(hx.debug_trace(q, p, sub)["cells"], hx.debug_trace(q, p)["cells"]), f"q{i}: the subset changed the cells"
        o = ox.search(q, to_oracle_params(p), sub, trace=True)
        assert o.trace.used_batched
        assert_ranking_close(r.passage_ids, r.scores, o.passage_ids, o.scores, RTOL_F32, f"batched q{i} vs oracle")


def test_large_k_probe_with_eligibility():
    """K = 131072 is the smallest K whose group maxima leave probe_mark_kernel<4>'s LDS form: probe_mark_kernel<8> with one
    eligible bitmap per query, on the dense path.  Checked against the single calls only."""
    spec = synth.SynthSpec(num_docs=20_000, num_centroids=131072, dim=128, nbits=2, doc_len_min=20, doc_len_max=60, seed=1241)
    cen = synth.centroids(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen, max_batch=8, n_contexts=1)
    qs, _ = synth.make_queries(spec, 4, n_tokens=32, cen=cen)
    rng = np.random.default_rng(7)
    subsets = [np.sort(rng.choice(20_000, 10_000, replace=False)).astype(np.int64),
               np.sort(rng.choice(20_000, 200, replace=False)).astype(np.int64), None, np.array([3, 777, 19_999], np.int64)]
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=8, centroid_score_threshold=None, centroid_batch_size=0)
    cells = [hx.debug_trace(q, p, s)["cells"].size for q, s in zip(qs, subsets)]
    assert len(set(cells)) >= 3, f"cell counts {cells}: the subsets do not separate the queries' probes"
    res = check_against_singles(hx, qs, p, subsets, "K=131072")
    assert all(r.passage_ids.size > 0 for r in res)
    assert set(res[3].passage_ids.tolist()) <= {3, 777, 19_999}
    hx.close()


@pytest.mark.parametrize("G", [2, 3])
def test_inprocess_shards_with_subsets(G):
    """Sharded: the eligible bitmaps of all subsets cross the shards in one exchange; subsets that live mostly in one shard."""
    import torch
    from next_plaid_amd.dist import HipShardBackend, ShardedSearcher
    spec, a = make_arrays(num_docs=6000, num_centroids=1024, dim=128, nbits=4, doc_len_min=5, doc_len_max=80, seed=55)
    full = hip_index(a)
    shards = [hip_index(a, shard_rank=r, shard_count=G) for r in range(G)]
    stream = torch.cuda.Stream()
    ss = ShardedSearcher([HipShardBackend(s, stream=stream) for s in shards], use_dist=False)
    qs, _ = synth.make_queries(spec, 8, n_tokens=32, cen=a["centroids"])
    first, last = np.arange(100, 900, dtype=np.int64), np.arange(5500, 6000, dtype=np.int64)
    subsets = [first, None, last, np.array([3, 5999, 7000, -1, 2500], np.int64), first, np.zeros(0, np.int64),
               np.arange(0, 6000, 7, dtype=np.int64), last]
    for cbs in (100_000, 300):
        p = P(n_full_scores=128, top_k=10, n_ivf_probe=4, centroid_score_threshold=None, centroid_batch_size=cbs)
        res = ss.search_batch(qs, p, subsets=subsets)
        ref = full.search_batch(qs, p, subsets=subsets)
        for i, (r, f) in enumerate(zip(res, ref)):
            assert np.array_equal(r.passage_ids, f.passage_ids), f"G={G} cbs={cbs} q{i}: {r.passage_ids} vs {f.passage_ids}"
            assert np.allclose(r.scores, f.scores, rtol=5e-5, atol=0), f"G={G} cbs={cbs} q{i} scores"
    with pytest.raises(ValueError):
        ss.search_batch(qs, p, subset=first, subsets=subsets)


def test_c_level_sharded_entry_world1_with_subsets():
    from next_plaid_amd.dist import CShardedSearcher, ShardComm
    spec, a = make_arrays(num_docs=3000, num_centroids=512, dim=128, nbits=4, doc_len_min=5, doc_len_max=60, seed=57)
    hx = hip_index(a)
    qs, _ = synth.make_queries(spec, 6, n_tokens=32, cen=a["centroids"])
    fifth = np.arange(0, 3000, 5, dtype=np.int64)
    subsets = [fifth, None, np.arange(40, dtype=np.int64), np.zeros(0, np.int64), fifth, np.array([2999, 3000, -2], np.int64)]
    comm = ShardComm(hx, 0, 1, rccl=False)
    cs = CShardedSearcher(hx, comm)
    for p in (P(n_full_scores=128, top_k=10, n_ivf_probe=8), P(n_full_scores=64, top_k=20, n_ivf_probe=4, centroid_batch_size=100)):
        got = cs.search_batch(qs, p, subsets=subsets)
        for i, (r, f) in enumerate(zip(got, hx.search_batch(qs, p, subsets=subsets))):
            assert np.array_equal(r.passage_ids, f.passage_ids), f"q{i}"
            assert np.allclose(r.scores, f.scores, rtol=5e-5, atol=0), f"q{i} scores"
    comm.close()


def test_invalid_arguments_leave_the_handle_usable(small):
    spec, a, ox, hx, qs = small
    p = P(n_full_scores=64, top_k=5, n_ivf_probe=4)
    q3 = qs[:3]
    ids = np.arange(10, dtype=np.int64)
    good = (ids, np.array([0, 4, 10], np.int64), np.array([0, -1, 1], np.int32))
    want = hx.search_batch_csr(q3, p, *good)
    for r, sub in zip(want, (ids[:4], None, ids[4:])):
        assert same_bits(r, hx.search(q3[r.query_id], p, sub))
    bad = {
        "offsets do not start at 0": (ids, np.array([1, 4, 10], np.int64), good[2]),
        "offsets decrease": (ids, np.array([0, 6, 4], np.int64), good[2]),
        "entry below -1": (ids, good[1], np.array([0, -2, 1], np.int32)),
        "entry >= n_subsets": (ids, good[1], np.array([0, 2, 1], np.int32)),
        "NULL ids with a positive count": (None, good[1], good[2]),
        "NULL query_subset with subsets": (ids, good[1], None),
    }
    for what, args in bad.items():
        with pytest.raises(ValueError) as e:
            hx.search_batch_csr(q3, p, *args)
        assert str(e.value), what
        for r, f in zip(hx.search_batch_csr(q3, p, *good), want):   # the handle still answers, and the same
            assert same_bits(r, f), what
    # NULL offsets with a positive subset count reach the library only from C: the mirror derives the count from the offsets
    import ctypes as C
    rc = api.lib().np_hip_search_batch_subsets(hx._h, None, None, 0, 128, C.byref(p._c()), None, None, 2, None, None, None, None, None)
    assert rc == 8 and "subset_offsets is NULL" in api.last_error()
    with pytest.raises(ValueError):
        hx.search_batch(q3, p, subset=ids, subsets=[None] * 3)
    with pytest.raises(ValueError):
        hx.search_batch(q3, p, subsets=[None] * 2)


CPP = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "next_plaid.hpp"
// argv: index dir, queries file (n, tokens, dim as i64, then f32 rows), output file, mode (gpu | cpu)
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
  std::vector<int64_t> evens, head, none;
  for (int64_t d = 0; d < 2000; d += 2) evens.push_back(d);
  for (int64_t d = 0; d < 100; ++d) head.push_back(d);
  std::vector<const std::vector<int64_t>*> subsets(n, nullptr);
  const std::vector<int64_t>* cyc[4] = {&evens, nullptr, &head, &none};
  for (size_t i = 0; i < n; ++i) subsets[i] = cyc[i % 4];
  int cpu_calls = 0;
  if (!std::strcmp(argv[4], "cpu"))   // the CPU hand-off takes one subset per call: one call per query
    next_plaid::set_cpu_fallback([&](const std::string&, const next_plaid::Query* q, size_t m, size_t, const next_plaid::SearchParameters&,
                                     bool, const std::vector<int64_t>* sub) {
      std::vector<next_plaid::QueryResult> out(m);
      for (size_t i = 0; i < m; ++i) {
        out[i].passage_ids = {(int64_t)(q[i].data - q[0].data), sub ? (int64_t)sub->size() : -1, (int64_t)cpu_calls};
        out[i].scores = {0.f, 0.f, 0.f};
      }
      ++cpu_calls;
      return out;
    });
  try {
    auto ix = next_plaid::MmapIndex::load(argv[1]);
    next_plaid::SearchParameters p;
    p.n_full_scores = 256;
    p.top_k = 10;
    p.n_ivf_probe = 4;
    p.centroid_score_threshold = std::nullopt;
    auto res = ix.search_batch_subsets(qs.data(), n, p, true, subsets);
    FILE* o = std::fopen(argv[3], "wb");
    for (auto& r : res) {
      int64_t c[2] = {(int64_t)r.query_id, (int64_t)r.passage_ids.size()};
      std::fwrite(c, 8, 2, o);
      std::fwrite(r.passage_ids.data(), 8, r.passage_ids.size(), o);
      std::fwrite(r.scores.data(), 4, r.scores.size(), o);
    }
    std::fclose(o);
    if (!std::strcmp(argv[4], "cpu") && cpu_calls != (int)n) return 3;
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  return 0;
}
"""


def test_cpp_mirror_gives_the_same_bytes(small, tmp_path):
    spec, a, ox, hx, qs = small
    src = tmp_path / "subsets_cli.cpp"
    src.write_text(CPP)
    exe = tmp_path / "subsets_cli"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", str(exe), "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), a, chunk_docs=700)
    with open(tmp_path / "q.bin", "wb") as f:
        f.write(np.array([len(qs), 16, 128], np.int64).tobytes() + np.concatenate(qs, 0).astype(np.float32).tobytes())
    subprocess.check_call([str(exe), str(ixdir), str(tmp_path / "q.bin"), str(tmp_path / "out.bin"), "gpu"])
    pool = subset_pool(2000)
    cyc = [pool["evens"], None, pool["head"], pool["empty"]]
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
    want = b""
    for r in npa.MmapIndex.load(str(ixdir)).search_batch(qs, p, subsets=[cyc[i % 4] for i in range(len(qs))]):
        want += np.array([r.query_id, r.passage_ids.size], np.int64).tobytes() + r.passage_ids.tobytes() + r.scores.tobytes()
    assert open(tmp_path / "out.bin", "rb").read() == want
    # the CPU hand-off: one hook call per query, each with its own subset
    env = dict(os.environ, NEXT_PLAID_FORCE_CPU="1")
    subprocess.check_call([str(exe), str(ixdir), str(tmp_path / "q.bin"), str(tmp_path / "cpu.bin"), "cpu"], env=env)
    raw = np.frombuffer(open(tmp_path / "cpu.bin", "rb").read(), np.uint8)
    rec = 16 + 3 * 8 + 3 * 4
    assert raw.size == rec * len(qs)
    for i in range(len(qs)):
        qid, cnt, off, sub_len, call = np.frombuffer(raw[i * rec: i * rec + 40].tobytes(), np.int64)
        assert (qid, cnt, off, call) == (i, 3, 0, i) and sub_len == [1000, -1, 100, 0][i % 4]


def test_device_entry_slices_and_out_of_range_entries(small):
    """np_hip_search_batch_subsets_device on torch tensors: max_batch = 3 cuts the eight queries into three passes, each reading
    its own part of the device-side map, and a `query_subset` entry outside [0, n_subsets) reads as -1 (the host cannot check an
    array that lives on the device).  Equal to the host entry, bit for bit."""
    import ctypes as C
    import torch
    spec, a, ox, _, qs = small
    hx = hip_index(a, max_batch=3)
    pool = subset_pool(2000)
    subsets = [pool["head"], None, pool["evens"], pool["evens"], pool["empty"], pool["odd_ids"], None, pool["head"]]
    ids, off, qsub = api.pack_subsets(subsets, 8)
    p = P(n_full_scores=256, top_k=10, n_ivf_probe=4, centroid_score_threshold=None)
    want = hx.search_batch(qs, p, subsets=subsets)
    assert any(r.passage_ids.size == 10 for r in want)
    dev = torch.device("cuda", 0)
    qoff = np.arange(9, dtype=np.int32) * 16
    d_q = torch.from_numpy(np.concatenate(qs, 0).astype(np.float32)).to(dev)
    d_qoff, d_ids, d_off = torch.from_numpy(qoff).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(off).to(dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    for wild in (False, True):
        m = qsub.copy()
        if wild:   # "none", spelled with entries the device clamps
            m[1], m[6] = 7, -5
        d_qsub = torch.from_numpy(m).to(dev)
        o_ids = torch.zeros((8, 10), dtype=torch.int64, device=dev)
        o_sc = torch.zeros((8, 10), dtype=torch.float32, device=dev)
        o_cnt = torch.zeros(8, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        api._check(api.lib().np_hip_search_batch_subsets_device(
            hx._h, ptr(d_q), ptr(d_qoff), qoff.ctypes.data_as(C.c_void_p), 8, 128, C.byref(p._c()), ptr(d_ids), ptr(d_off),
            off.ctypes.data_as(C.c_void_p), off.size - 1, ptr(d_qsub), ptr(o_ids), ptr(o_sc), ptr(o_cnt), None))
        torch.cuda.synchronize()
        g_ids, g_sc, g_cnt = o_ids.cpu().numpy(), o_sc.cpu().numpy(), o_cnt.cpu().numpy()
        for i, r in enumerate(want):
            assert g_cnt[i] == r.passage_ids.size, f"wild={wild} q{i}: count {g_cnt[i]} vs {r.passage_ids.size}"
            assert np.array_equal(g_ids[i, : g_cnt[i]], r.passage_ids), f"wild={wild} q{i}"
            assert np.array_equal(g_sc[i, : g_cnt[i]].view(np.uint32), r.scores.view(np.uint32)), f"wild={wild} q{i} scores"
    # the offsets are checked on the host here too; a NULL device copy is refused
    rc = api.lib().np_hip_search_batch_subsets_device(
        hx._h, ptr(d_q), ptr(d_qoff), qoff.ctypes.data_as(C.c_void_p), 8, 128, C.byref(p._c()), ptr(d_ids), None,
        off.ctypes.data_as(C.c_void_p), off.size - 1, ptr(d_qsub), ptr(o_ids), ptr(o_sc), ptr(o_cnt), None)
    assert rc == 8 and "device copy" in api.last_error()
    hx.close()
