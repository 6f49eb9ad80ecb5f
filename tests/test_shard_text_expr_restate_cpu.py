"""The sharded keyword search over tree queries restated (tests/shard_text_expr_restate.py): the protocol equals the search
over the whole table bit for bit, the fixture corpus provably holds every case the sharded counts can get wrong, every planted
defect changes a result, and the host code that sizes the counting exchange and groups the counting pre-pass
(np_text_plan.h) stands alone.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from next_plaid_amd import text as T
import shard_text_expr_restate as X
import shard_text_restate as S

TOP_KS = [1, 10, 1024]
N = X.N_CPU


@pytest.fixture(scope="module")
def table():
    texts = X.corpus_texts(N)
    data = T.TextIndexData.from_texts(texts)
    rs = X.RestatedExpr(data, N)
    names = [n for n, _ in X.special_trees(data)]
    exprs = X.special_exprs(data)
    found = S.find_f32_collision(rs, data, N, [2, 3])
    if found is not None:
        names.append("f32 collision")
        exprs.append(T.TextExpr.from_query(found[0]))
    whole = [rs.expr_scores(e) for e in exprs]
    return texts, data, rs, names, exprs, whole, found


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_the_corpus_is_what_it_says(table):
    texts, data, rs, names, exprs, whole, found = table
    v = data.vocab
    assert data.n_rows == N and N % 2 == 1
    at = names.index
    lef, mid = T.prefix_range("lef", data), T.prefix_range("mid", data)
    assert lef[1] - lef[0] == 2 and mid[1] - mid[0] == 2 and T.prefix_range("zz", data)[1] <= T.prefix_range("zz", data)[0]
    one = T.prefix_range("lefa", data)
    assert one[1] - one[0] == 1
    first = rs.doc_len[: N // 2]
    planted = {b for _, b in X.tie_pairs(N)} | {N // 2}
    second = np.asarray([rs.doc_len[d] for d in range(N // 2, N) if d not in planted])
    assert first.max() < second.min()                                  # lengths differ systematically between the halves
    for G in (2, 3):
        sh = X.ShardedExpr(rs, N, G)
        rg = sh.ranges
        # a prefix range whose documents all lie on one shard
        per = sh.shard_hits([lef[0]], lef)
        assert per[0] > 0 and sum(per[1:]) == 0
        # a document holding two terms of one range: nHit is below the sum of the document frequencies
        for r in (lef, mid):
            f, over = sh._phrase((r[0],), r)
            assert any(d in rs.post[r[0]] and d in rs.post[r[0] + 1] for d in f) and len(f) < over
        # a term of the range that a shard lacks, while the shard holds another one
        assert not any(rg[0][0] <= d < rg[0][1] for d in rs.post[v["midb"]])
        assert any(rg[0][0] <= d < rg[0][1] for d in rs.post[v["mida"]])
        # several tokens ending in a prefix: no hit on the first shard, though it holds the first token and the range's terms
        per = sh.shard_hits([v["alpha"], mid[0]], mid)
        assert per[0] == 0 and sum(per) > 0 and any(rg[0][0] <= d < rg[0][1] for d in rs.post[v["alpha"]])
        per = sh.shard_hits([v["wo1"], mid[0]], mid)
        assert min(per) > 0 and len(set(per)) > 1                      # ... and one that every shard counts, unevenly
        # a NOT that empties one shard whose left side is not empty there
        sc = whole[at("nota NOT notb")]
        assert sc and not any(rg[0][0] <= d < rg[0][1] for d in sc)
        assert any(rg[0][0] <= d < rg[0][1] for d in rs.post[v["nota"]])
        # a shard whose list is shorter than top_k while the merged result is full
        got = sh.search(exprs[at("lef*")], 10)
        assert got[0].size == 10 and min(sh.last_lengths) < 10
        for a, b in X.tie_pairs(N):
            assert texts[a] == texts[b] and a < rg[0][1] and b >= rg[-1][0]
    sc = whole[at("tie")]
    assert all(sc[a] == sc[b] for a, b in X.tie_pairs(N))              # exact f64 ties
    # every term's prefix is every document with a token
    assert len(whole[at("every term")]) == int(np.count_nonzero(rs.doc_len))


def test_the_count_vector_follows_from_the_queries(table):
    texts, data, rs, names, exprs, whole, found = table
    multi, prefix = X.counted_phrases(exprs)
    assert len(multi) >= 5 and len(prefix) >= 8
    at = names.index("nowhere mid* OR mid*")
    assert (at, 0) not in multi and (at, 1) in prefix                  # an unknown token: not counted
    at = names.index("zz*")
    assert (at, 0) not in prefix                                       # an empty range: not counted


@pytest.mark.parametrize("G", X.GS)
def test_the_protocol_equals_the_whole_table(table, G):
    texts, data, rs, names, exprs, whole, found = table
    sh = X.ShardedExpr(rs, N, G)
    some = np.arange(0, N, 3)
    odd = np.array([3, N - 2, N - 1, 7000, -1, 3, 750, 750, 10, N - 11], np.int64)      # outside the range, duplicates
    n_hits = 0
    for qi, e in enumerate(exprs):
        for k in TOP_KS:
            want = X.RestatedExpr.rank(whole[qi], k)
            assert same(sh.search(e, k), want), (G, names[qi], k)
            n_hits += want[0].size
        for sub in (some, odd, np.zeros(0, np.int64)):
            keep = sub[(sub >= 0) & (sub < N)]
            assert same(sh.search(e, 10, subset=sub), X.RestatedExpr.rank(whole[qi], 10, keep)), (G, names[qi])
    assert n_hits > 0


def test_every_planted_defect_changes_a_result(table):
    """With any of these mistakes in the implementation at least one result of the special queries differs, at EVERY G the GPU
    test runs (the f32 merge: at some G)."""
    texts, data, rs, names, exprs, whole, found = table
    for G in (2, 3):
        sh = X.ShardedExpr(rs, N, G)
        for defect in X.DEFECTS:
            if defect == "f32":
                continue
            changed = [(names[qi], k) for qi, e in enumerate(exprs) for k in TOP_KS
                       if not same(sh.search(e, k, defect=defect), X.RestatedExpr.rank(whole[qi], k))]
            assert changed, f"G={G}: the corpus cannot see the defect {defect!r}"
    assert found is not None, "no f32 collision on this corpus"
    q, hi_doc, lo_doc = found
    sc = whole[-1]
    assert sc[hi_doc] > sc[lo_doc] and np.float32(sc[hi_doc]) == np.float32(sc[lo_doc]) and hi_doc > lo_doc
    seen = False
    for G in (2, 3):
        sh = X.ShardedExpr(rs, N, G)
        seen = seen or not same(sh.search(exprs[-1], 1024, defect="f32"), X.RestatedExpr.rank(sc, 1024))
    assert seen, "a merge on f32 scores must put the pair the wrong way round at some G"


def test_a_flat_query_lifted_to_a_tree_keeps_its_scores(table):
    texts, data, rs, names, exprs, whole, found = table
    for q in S.special_queries(data)[:6]:
        flat = rs.scores(q)
        tree = rs.expr_scores(T.TextExpr.from_query(q))
        assert flat.keys() == tree.keys() and all(flat[d] == tree[d] for d in flat)


def test_host_code_of_the_counting_pre_pass_stands_alone(tmp_path):
    """tests/cpp/text_expr_counts_check.cpp: text_counted_expr_phrases and the grouping of the counting pre-pass
    (np_text_plan.h) with the host compiler alone (no device, no library), plain and under AddressSanitizer + UBSan."""
    src = os.path.join(ROOT, "tests", "cpp", "text_expr_counts_check.cpp")
    inc = os.path.join(ROOT, "next-plaid_amd", "csrc")
    for name, flags in (("plain", ["-O1"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = tmp_path / f"text_expr_counts_check_{name}"
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I", inc, src, "-o", str(exe)])
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "all checks passed" in out.stdout, name + ": " + out.stdout + out.stderr
