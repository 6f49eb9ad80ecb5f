"""np_hip_maxsim_batch_long_i8 (np_maxsim_long_i8.hip): int8 rows for queries past 256 tokens against
tests/maxsim_i8_restate.py pair(), bit for bit -- scores as uint32 views, sims and positions -- in every dim class x form x
entry; the tie, NaN and infinity rules; and the bits of np_hip_maxsim_batch_i8 for the queries that fit it.  No tolerance
anywhere: the rule is exact integers and single f32 roundings."""
import functools
import itertools

import numpy as np
import pytest

import maxsim_i8_restate as R
from test_gpu_maxsim_batch import u32

import next_plaid_amd as npa
from maxsim import maxsim_long as ML

pytestmark = pytest.mark.gpu
N_DOCS = 348   # 6 queries x ceil(348 / 4) workgroups reach twice the 256 compute units: four documents share a workgroup
# a repeated id, an empty list, every document in reverse (four pairs a workgroup in the listed form too), ...
LISTS = [[3, 3, 1], [], list(range(N_DOCS))[::-1], [0, 1, 2, 3], [3, 2, 1, 0, 3], [2, 3, 3, N_DOCS - 1]]


def codes_scales(g, n, dim):
    """Codes in [-127, 127]: |dot| <= 1024 * 127 * 127 < 2^24, as the restatement requires."""
    return g.integers(-127, 128, (n, dim)).astype(np.int8), g.uniform(0.001, 2.0, n).astype(np.float32)


def run(q, d, entry, **kw):
    """maxsim_scores_long_i8 of [(codes, scales)] lists with matches: numpy through the host entry, torch tensors through the
    device entry.  Returns numpy (scores, sims, positions) per query."""
    if entry == "device":
        import torch
        q, d = ([tuple(torch.from_numpy(a).cuda() for a in x) for x in xs] for xs in (q, d))
    out = ML.maxsim_scores_long_i8([x[0] for x in q], [x[0] for x in d], [x[1] for x in q], [x[1] for x in d], return_matches=True, **kw)
    return [tuple(a.cpu().numpy() for a in o) for o in out] if entry == "device" else out


def same(got, k, ref):
    """row k of a query's (scores, sims, positions) has the restatement's bits"""
    return u32(got[0][k]) == u32(ref[0]) and np.array_equal(u32(got[1][k]), u32(ref[1])) and np.array_equal(got[2][k], ref[2])


@functools.lru_cache(None)
def batch(dim):
    """Queries of 0, 5, 256, 257, 300 and 545 tokens (545: 18 tiles, three passes at 8 a pass, nine at dim 1024's 2); documents
    of 0, 31, 33 and 300 tokens in one workgroup, then tiny ones; the restatement of every pair."""
    g = np.random.default_rng(900 + dim)
    q = [codes_scales(g, n, dim) for n in (0, 5, 256, 257, 300, 545)]
    d = [codes_scales(g, n, dim) for n in (0, 31, 33, 300)] + [codes_scales(g, n, dim) for n in g.choice([0, 1, 3], N_DOCS - 4)]
    return q, d, {(i, j): R.pair(*q[i], *d[j]) for i, j in itertools.product(range(len(q)), range(N_DOCS))}


@pytest.mark.parametrize("entry", ("host", "device"))
@pytest.mark.parametrize("form", ("all", "listed"))
@pytest.mark.parametrize("dim", (40, 128, 160, 1024))
def test_every_pair_has_the_bits_of_the_restatement(dim, form, entry):
    """40: byte loads and a padded step; 128: one chunk of 16-byte loads; 160: a partial second chunk; 1024: eight chunks and
    passes of two tiles."""
    q, d, ref = batch(dim)
    out = run(q, d, entry, pairs=LISTS if form == "listed" else None)
    for i in range(len(q)):
        ids = LISTS[i] if form == "listed" else range(N_DOCS)
        assert out[i][0].shape == (len(ids),)
        assert all(same(out[i], k, ref[i, j]) for k, j in enumerate(ids)), (i, [j for k, j in enumerate(ids) if not same(out[i], k, ref[i, j])][:8])


def test_ties_and_non_finite_scales():
    """Rows 2 and 40 of document 0 are equal and larger than every other row for every query token (the codes of the query
    are positive): a tie across two waves' tiles, the lowest position wins.  Row 5 would be larger still, but its scale is
    NaN.  A NaN and an infinite query scale: 0.0 / -1, nothing added.  Ids outside [0, n_docs) reach the device entry only
    and score NaN."""
    g = np.random.default_rng(77)
    (cq, sq), d = codes_scales(g, 300, 128), [codes_scales(g, 70, 128), codes_scales(g, 33, 128)]
    cq = np.abs(cq) + (cq == 0)
    d[0][0][[2, 5, 40]], d[0][1][[2, 40]], d[0][1][5] = 127, 3.0, np.nan
    sq[7], sq[260] = np.nan, np.inf
    sc, sims, pos = run([(cq, sq)], d, "device", pairs=[[0, 1, 7, -1]])[0]
    assert same((sc, sims, pos), 0, R.pair(cq, sq, *d[0])) and same((sc, sims, pos), 1, R.pair(cq, sq, *d[1]))
    ok = np.ones(300, bool)
    ok[[7, 260]] = False
    assert np.all(pos[0][ok] == 2) and np.all(pos[:2, ~ok] == -1) and np.all(sims[:2, ~ok] == 0)
    assert np.isnan(sc[2:]).all() and np.all(pos[2:] == -1) and np.all(sims[2:] == 0)


def test_a_short_query_has_the_bits_of_maxsim_batch_i8():
    q, d, _ = batch(160)
    q, d = q[1:3], d[:40]                   # 5 and 256 tokens
    a = run(q, d, "host")
    b = npa.maxsim_scores([x[0] for x in q], [x[0] for x in d], query_scales=[x[1] for x in q], document_scales=[x[1] for x in d], return_matches=True)
    for x, y in zip(a, b):
        assert all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(x, y))
