"""np_hip_maxsim_batch_long (np_maxsim_long.hip): queries past 256 tokens, every mode x form x entry.  Integer rows against
int64 numpy exactly (scores and first-argmax positions), float rows against the float64 reference and the derived bound of
tests/maxsim_restate.py (no tolerance is measured), a pair's bits against np_hip_maxsim_batch and against its surroundings,
and the non-finite rules."""
import functools
import itertools

import numpy as np
import pytest

import maxsim_restate as M
from test_gpu_maxsim_batch import u32

import next_plaid_amd as npa
from maxsim import maxsim_long as ML

pytestmark = pytest.mark.gpu
CASES = list(itertools.product(M.MODES, ("all", "listed"), ("host", "device")))
case = pytest.mark.parametrize("mode,form,entry", CASES, ids=["-".join(c) for c in CASES])


def run(q, d, mode, form, entry, pairs=None, matches=False, fn=None):
    """maxsim_scores_long in `mode` (bf16 rows as uint16 words / torch.bfloat16), numpy through the host entry or torch through
    the device entry.  form "listed" without `pairs`: every query lists all documents in reverse, and the result is put back
    into document order.  Returns numpy: per query its scores, or (scores, sims, positions)."""
    import torch
    if mode == "bf16_rows":
        q, d = ([(M.bf16(x).view(np.uint32) >> 16).astype(np.uint16) for x in xs] for xs in (q, d))
    if entry == "device":
        to = lambda x: torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16) if x.dtype == np.uint16 else torch.from_numpy(x).cuda()  # noqa: E731
        q, d = [to(x) for x in q], [to(x) for x in d]
    rev = pairs is None and form == "listed"
    if rev:
        pairs = [np.arange(len(d))[::-1]] * len(q)
    out = (fn or ML.maxsim_scores_long)(q, d, pairs=pairs, precision=0 if mode == "f32" else 3, return_matches=matches)
    if entry == "device":
        torch.cuda.synchronize()
    host = lambda o: (o.cpu().numpy() if entry == "device" else o)[::-1 if rev else 1]   # noqa: E731
    return [tuple(host(x) for x in o) if matches else host(o) for o in out]


@functools.lru_cache(None)
def planted():
    """Rows of integers in [-4, 4] at dim 40 (|dot| <= 640: exact in every mode) with int64 numpy's scores, maxima and first
    argmax.  Query 545's last token and document 130's last token are all 4s: 640 is reached there only."""
    g = np.random.default_rng(5)
    q = [g.integers(-4, 5, (n, 40)).astype(np.float32) for n in (0, 1, 129, 257, 288, 289, 545)]
    d = [g.integers(-4, 5, (n, 40)).astype(np.float32) for n in (0, 1, 33, 130)]
    q[-1][544] = d[-1][129] = 4
    ref = {}
    for (i, x), (j, y) in itertools.product(enumerate(q), enumerate(d)):
        s = x.astype(np.int64) @ y.astype(np.int64).T
        best = s.max(1) if y.shape[0] else np.zeros(x.shape[0], np.int64)
        ref[i, j] = (best.sum(), best, s.argmax(1) if y.shape[0] else np.full(x.shape[0], -1))
    return q, d, ref


@case
def test_integer_rows_are_exact(mode, form, entry):
    q, d, ref = planted()
    out = run(q, d, mode, form, entry, matches=mode == "f32")
    for i, j in ref:
        score, best, arg = ref[i, j]
        sc = out[i][0] if mode == "f32" else out[i]
        assert float(sc[j]) == score, (i, j, sc[j], score)
        if mode == "f32":
            assert np.array_equal(out[i][1][j], best) and np.array_equal(out[i][2][j], arg), (i, j)
    assert mode != "f32" or out[-1][2][3][544] == 129


@functools.lru_cache(None)
def floats(dim):
    g = np.random.default_rng(400 + dim)
    return [M.unit_rows(g, n, dim) for n in (300, 257, 40)], [M.unit_rows(g, n, dim) for n in (0, 31, 300)]


@case
@pytest.mark.parametrize("dim", (37, 128, 160))
def test_float_rows_within_the_bound(dim, mode, form, entry):
    """37: element loads with a pad; 128: 16-byte loads; 160: several chunks with a remainder in both chunk sizes."""
    q, d = floats(dim)
    if mode == "bf16_rows":
        q, d = [M.bf16(x) for x in q], [M.bf16(x) for x in d]
    out = run(q, d, mode, form, entry, matches=mode == "f32")
    worst = 0.0
    for i, j in itertools.product(range(len(q)), range(len(d))):
        r = M.pair(q[i], d[j], mode)
        sc = out[i][0] if mode == "f32" else out[i]
        err = abs(float(sc[j]) - r["score"])
        worst = max(worst, err / max(r["bound"], 1e-300))
        assert err <= r["bound"], (i, j, err, r["bound"])
        if mode == "f32":
            sims, pos = out[i][1][j], out[i][2][j]
            tot = np.float32(0)
            for x in sims:
                tot = np.float32(tot + x)
            assert u32(tot) == u32(sc[j]) and np.array_equal(pos >= 0, r["has"])
            t = np.nonzero(r["has"])[0]
            assert np.all(np.abs(sims[t] - r["sims"][t, pos[t]]) <= r["tb"][t, pos[t]])
    print(f"dim {dim} {mode} {form} {entry}: max |err| / bound {worst:.3f}")


@case
def test_a_short_query_has_the_bits_of_maxsim_batch(mode, form, entry):
    g = np.random.default_rng(8)
    q, d = [M.unit_rows(g, n, 72) for n in (256, 33, 5)], [M.unit_rows(g, n, 72) for n in (17, 300, 129)]
    a = run(q, d, mode, form, entry, matches=mode == "f32")
    # api.maxsim_scores takes bf16 rows as device tensors only; the bits do not depend on the entry
    b = run(q, d, mode, form, "device" if mode == "bf16_rows" else entry, matches=mode == "f32", fn=npa.maxsim_scores)
    for x, y in zip(a, b):
        for u, v in zip(x, y) if mode == "f32" else ((x, y),):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


@functools.lru_cache(None)
def crowd():
    """A 545-token query beside a 40- and a 300-token one; 700 documents, enough for 4 pairs per workgroup in both forms."""
    g = np.random.default_rng(9)
    lens = np.r_[g.choice([0, 1, 20, 33], 699), 130][g.permutation(700)]
    return [M.unit_rows(g, n, 40) for n in (40, 545, 300)], [M.unit_rows(g, n, 40) for n in lens], int(np.argmax(lens))


@case
def test_a_long_query_is_independent_of_its_surroundings(mode, form, entry):
    q, d, big = crowd()
    ks, m = [big, 0, 3, 699], mode == "f32"
    alone = [run([q[1]], [d[k]], mode, "all", "host", matches=m)[0] for k in ks]
    if form == "all":
        got, at = run(q, d, mode, form, entry, matches=m)[1], ks
    else:                                   # a repeated and a reordered id in front of every document in reverse
        ids = np.r_[ks[2], ks[0], ks[2], np.arange(700)[::-1]]
        got, at = run(q, d, mode, form, entry, pairs=[ids[:5], ids, ids[:9]], matches=m)[1], [1, 3 + 699, 0, 3]
    for a, k in zip(alone, at):
        for u, v in zip(a, got) if m else ((a, got),):
            assert np.array_equal(u[0].view(np.uint32), v[k].view(np.uint32)), k
    assert form == "all" or not m or np.array_equal(got[1][0], got[1][2])


@case
def test_non_finite(mode, form, entry):
    g = np.random.default_rng(10)
    q, d = [M.unit_rows(g, 330, 40)], [M.unit_rows(g, 70, 40), M.unit_rows(g, 33, 40)]
    q[0][300] = np.nan                      # adds nothing, matches nothing
    d[1][:, 0] = np.inf                     # every sim of this document is non-finite
    m = mode == "f32"
    pairs = [[0, 1, 7, -1]] if entry == "device" and form == "listed" else None   # ids outside [0, n_docs): the device entry only
    out = run(q, d, mode, form, entry, pairs=pairs, matches=m)[0]
    sc = out[0] if m else out
    qz = q[0].copy()
    qz[300] = 0                             # the reference of a token that adds nothing: a zero row, whose maximum and bound are 0
    r = M.pair(M.bf16(qz) if mode == "bf16_rows" else qz, M.bf16(d[0]) if mode == "bf16_rows" else d[0], mode)
    assert abs(float(sc[0]) - r["score"]) <= r["bound"] and sc[1] == 0
    assert pairs is None or np.isnan(sc[2:]).all()
    if m:
        assert out[2][0][300] == -1 and out[1][0][300] == 0 and np.all(out[2][0][:300] >= 0)
        assert np.all(out[2][1:] == -1) and np.all(out[1][1:] == 0)
