"""The sharded keyword search restated (tests/shard_text_restate.py): the protocol equals the search over the whole table, the
fixture corpus tells a wrong implementation from a right one, the filter fixtures tell a local subset length from the global
one, and the host code of the exchanges (np_dist_plan.h) stands alone.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT, make_arrays

from next_plaid_amd import text as T
import shard_text_restate as S
import text_restate as R

GS = [1, 2, 3, 5]
GPU_GS = [2, 3]          # what tests/test_gpu_sharded_hybrid.py runs
TOP_KS = [1, 10, 1024]   # 1024: more than the matches of most queries


@pytest.fixture(scope="module")
def table():
    texts = S.corpus_texts()
    data = T.TextIndexData.from_texts(texts)
    rs = R.Restated(data, S.N_DOCS)
    queries = S.special_queries(data) + R.random_queries(data, 40, seed=3)
    whole = [rs.scores(q) for q in queries]
    return texts, data, rs, queries, whole


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_the_corpus_is_what_it_says(table):
    texts, data, rs, queries, whole = table
    n = S.N_DOCS
    assert data.n_rows == n and n % 2 == 1 and len(data.terms) < 48
    planted = {b for _, b in S.TIE_PAIRS} | {n // 2}
    first = rs.doc_len[: n // 2]
    second = np.asarray([rs.doc_len[d] for d in range(n // 2, n) if d not in planted])
    assert first.max() < second.min()                                   # lengths differ systematically between the halves
    v = data.vocab
    for G in GS[1:]:
        rg = S.shard_ranges(n, G)
        assert set(d // 1 for d in rs.post[v["lefty"]]) <= set(range(*rg[0]))        # one shard only
        assert set(rs.post[v["righty"]]) <= set(range(*rg[-1]))
        hits = rs.phrase_freqs([v["alpha"], v["beta"]])
        per = [sum(1 for d in hits if lo <= d < hi) for lo, hi in rg]
        assert min(per) > 0 and max(per) >= 4 * min(per)                # the phrase is split unevenly, and no shard lacks it
        assert len(hits) < len(rs.post[v["alpha"]])                     # its hit count is not a document frequency
        for a, b in S.TIE_PAIRS:
            assert texts[a] == texts[b] and a < rg[0][1] and b >= rg[-1][0]
    sc = whole[11]                                                      # "tie"
    assert all(sc[a] == sc[b] for a, b in S.TIE_PAIRS)                  # exact f64 ties


@pytest.mark.parametrize("G", GS)
def test_the_protocol_equals_the_whole_table(table, G):
    texts, data, rs, queries, whole = table
    sh = S.Sharded(rs, S.N_DOCS, G)
    some = np.arange(0, S.N_DOCS, 3)
    odd = np.array([3, 1499, 1500, 7000, -1, 3, 750, 750, 10, 1490], np.int64)      # outside the range, duplicates
    n_hits = 0
    for qi, q in enumerate(queries):
        for k in TOP_KS:
            want = R.Restated.rank(whole[qi], k)
            assert same(sh.search(q, k), want), (G, qi, k)
            n_hits += want[0].size
        for sub in (some, odd, np.zeros(0, np.int64)):
            keep = sub[(sub >= 0) & (sub < S.N_DOCS)]
            assert same(sh.search(q, 10, subset=sub), R.Restated.rank(whole[qi], 10, keep)), (G, qi)
    assert n_hits > 0


def test_every_planted_defect_changes_a_result_at_the_gpu_tests_sizes(table):
    """The GPU parity runs special_queries at top_k 1, 10 and 1024 on G = 2 and 3: with any of these mistakes in the
    implementation at least one of those results differs, at EVERY G the GPU test runs."""
    texts, data, rs, queries, whole = table
    special = S.special_queries(data)
    found = S.find_f32_collision(rs, data, S.N_DOCS, GPU_GS)
    for G in GPU_GS:
        sh = S.Sharded(rs, S.N_DOCS, G)
        for defect in S.DEFECTS:
            if defect == "f32":
                continue
            changed = [(qi, k) for qi, q in enumerate(special) for k in TOP_KS
                       if not same(sh.search(q, k, defect=defect), R.Restated.rank(whole[qi], k))]
            assert changed, f"G={G}: the corpus cannot see the defect {defect!r}"
    # two f64 scores that round to one f32, in different shards, the larger id scoring higher: found by a search over random
    # queries of this corpus (the GPU test runs the same query)
    assert found is not None, "no f32 collision on this corpus: drop the f32 defect from this test and from the GPU test"
    q, hi_doc, lo_doc = found
    sc = rs.scores(q)
    assert sc[hi_doc] > sc[lo_doc] and np.float32(sc[hi_doc]) == np.float32(sc[lo_doc]) and hi_doc > lo_doc
    seen = False
    for G in GPU_GS:
        sh = S.Sharded(rs, S.N_DOCS, G)
        assert same(sh.search(q, 1024), R.Restated.rank(sc, 1024))
        seen = seen or not same(sh.search(q, 1024, defect="f32"), R.Restated.rank(sc, 1024))
    assert seen, "a merge on f32 scores must put the pair the wrong way round at some G"


@pytest.mark.parametrize("G", GPU_GS)
def test_a_local_subset_length_gives_another_probe(G):
    """clamp(nprobe * N / len, nprobe, n_elig) from the global length of a filter's id list and from each shard's local one:
    they differ on every shard for both spread filters, with n_elig well above the globally scaled value -- otherwise the GPU
    parity of the filtered search would pass with the local length in the kernel."""
    spec, a = make_arrays(**S.GEOMETRY)
    rows = S.filter_rows()
    n, nprobe = S.N_DOCS, 4
    shares = []
    for cond in S.SPREAD_FILTERS:
        ids = S.filter_ids(cond, rows)
        n_elig = S.eligible_count(a, ids)
        glob = S.probe_scale(nprobe, n, ids.size, n_elig)
        assert nprobe < glob and 2 * glob <= n_elig, (cond, glob, n_elig)       # neither clamp decides the global value
        local = []
        for lo, hi in S.shard_ranges(n, G):
            own = ids[(ids >= lo) & (ids < hi)]
            assert own.size > 0                                                 # spread over all shards
            local.append(S.probe_scale(nprobe, n, own.size, n_elig))
        assert all(v != glob for v in local), (cond, glob, local)
        per = [int(((ids >= lo) & (ids < hi)).sum()) for lo, hi in S.shard_ranges(n, 2)]
        shares.append(per[0] / ids.size)
    assert abs(shares[0] - 0.5) < 0.01 and abs(shares[1] - 0.7) < 0.02          # one evenly, one roughly 70 / 30


def test_host_code_of_the_exchanges_stands_alone(tmp_path):
    """tests/cpp/dist_plan_check.cpp: np_dist_plan.h with the host compiler alone (no device, no library), plain and under
    AddressSanitizer + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "dist_plan_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"dist_plan_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr
