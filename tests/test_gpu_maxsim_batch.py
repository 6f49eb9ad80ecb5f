"""np_hip_maxsim_batch (np_maxsim.hip) against the float64 reference of tests/maxsim_restate.py, every score within the
derived bound (no tolerance is measured): the shape grid, independence of a pair from its surroundings, the matches at
precision 0, and the refusals."""
import numpy as np
import pytest

import maxsim_restate as M

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu

# 1, 20, 33, 128, 1024 and one value below, at and above each chunk (MAXSIM_CHUNK_F32 = 32, MAXSIM_CHUNK_BF16 = 64)
DIMS = sorted({1, 20, 33, 128, 1024} | {c + e for c in (api.MAXSIM_CHUNK_F32, api.MAXSIM_CHUNK_BF16) for e in (-1, 0, 1)})
LQ = (1, 32, 33, 256)
DOC_LENS = (0, 1, 31, 32, 33, 129, 1030)
LISTS = ([6, 0, 3, 6, 1], [5, 4, 3, 2, 1, 0], [2], [1, 5, 5, 6, 4, 0, 2, 3])       # repeats and out-of-order ids


def u32(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def run(q, d, mode, **kw):
    """maxsim_scores in `mode`: numpy through the host entry, bf16 rows as torch tensors through the device entry."""
    if mode == "bf16_rows":
        import torch
        to = lambda xs: [torch.from_numpy(M.bf16(x)).cuda().to(torch.bfloat16) for x in xs]   # noqa: E731 (exact: already bf16 values)
        out = npa.maxsim_scores(to(q), to(d), precision=3, **kw)
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out]
    return npa.maxsim_scores(q, d, precision=0 if mode == "f32" else 3, **kw)


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("dim", DIMS)
def test_shape_grid(dim, mode):
    g = np.random.default_rng(100 + dim)
    q = [M.unit_rows(g, n, dim) for n in LQ]
    d = [M.unit_rows(g, n, dim) for n in DOC_LENS]
    if mode == "bf16_rows":
        q, d = [M.bf16(x) for x in q], [M.bf16(x) for x in d]
    ref = {(i, j): M.pair(q[i], d[j], mode) for i in range(len(q)) for j in range(len(d))}
    listed, full = run(q, d, mode, pairs=LISTS), run(q, d, mode)
    for i in range(len(q)):
        assert full[i].shape == (len(d),)
        for got, j in list(zip(listed[i], LISTS[i])) + list(zip(full[i], range(len(d)))):
            r = ref[i, j]
            print(f"dim {dim} {mode} q{i} d{j}: |err| {abs(float(got) - r['score']):.3e} bound {r['bound']:.3e}")
            assert abs(float(got) - r["score"]) <= r["bound"]
        assert np.array_equal(u32(listed[i]), u32(full[i][LISTS[i]]))          # the two forms agree bit for bit


@pytest.mark.parametrize("mode", M.MODES)
def test_shared_workgroups(mode):
    """Calls large enough that the plan keeps 4 documents per workgroup (a 256-CU device asks for 512 workgroups first) and,
    in all-pairs form, 8 queries per group: short documents side by side in one workgroup with a long one among them, a
    3-tile query in 4 accumulator slots, B = 33 not a multiple of the group, 514 documents not a multiple of 4.  Every score
    within the bound; the two forms (1 and 8 queries per workgroup) and a pair scored alone give the same bits."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256       # else the plan splits these calls further
    g, dim = np.random.default_rng(11), 72
    d = [M.unit_rows(g, n, dim) for n in np.r_[g.choice([0, 1, 31, 33, 20], 513), 700][g.permutation(514)]]
    q = [M.unit_rows(g, n, dim) for n in g.integers(1, 33, 33)]
    qlong = [M.unit_rows(g, n, dim) for n in (70, 5, 32, 33, 96, 1, 64, 17)]          # listed: 3 tiles at most -> 4 slots
    if mode == "bf16_rows":
        q, qlong, d = ([M.bf16(x) for x in xs] for xs in (q, qlong, d))
    lists = [g.integers(0, 514, 260) for _ in qlong]                                   # repeats, any order
    full, listed, same = run(q, d, mode), run(qlong, d, mode, pairs=lists), run(q, d, mode, pairs=[np.arange(514)] * 33)
    for got, qs, ids in ((full, q, [np.arange(514)] * 33), (listed, qlong, lists)):
        score, bound = M.batch(qs, d, mode)
        for i in range(len(qs)):
            err = np.abs(got[i].astype(np.float64) - score[i][ids[i]])
            print(f"{mode} q{i}: max |err| / bound {np.max(err / np.maximum(bound[i][ids[i]], 1e-300)):.3f}")
            assert np.all(err <= bound[i][ids[i]])
    assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(full, same))
    for i, k in ((0, 3), (4, 259)):
        assert u32(run([qlong[i]], [d[lists[i][k]]], mode)[0])[0] == u32(listed[i])[k]


def test_shared_workgroups_matches():
    """The matches of a workgroup's second to fourth document: rows and positions equal the pair scored alone, bit for bit."""
    g, dim = np.random.default_rng(12), 40
    d = [M.unit_rows(g, n, dim) for n in g.choice([0, 1, 31, 33, 150], 300)]
    q = [M.unit_rows(g, n, dim) for n in (70, 5, 32, 33, 96, 1, 64, 17)]
    lists = [g.integers(0, 300, 260) for _ in q]
    out = npa.maxsim_scores(q, d, pairs=lists, return_matches=True)
    for i in range(len(q)):
        for k in (1, 2, 3, 130, 257, 259):
            sc, sims, pos = npa.maxsim_scores([q[i]], [d[lists[i][k]]], return_matches=True)[0]
            assert u32(sc)[0] == u32(out[i][0])[k] and np.array_equal(u32(sims[0]), u32(out[i][1][k]))
            assert np.array_equal(pos[0], out[i][2][k])


@pytest.mark.parametrize("precision", (0, 3))
def test_a_pair_is_independent_of_its_surroundings(precision):
    import torch
    g = np.random.default_rng(7)
    dim = 130
    qs = [M.unit_rows(g, n, dim) for n in (5, 256, 40, 33, 1, 64, 97)]
    ds = [M.unit_rows(g, n, dim) for n in (17, 300, 129, 2, 64)]
    kw = dict(precision=precision, return_matches=precision == 0)
    first = lambda o: o if precision else o[0]   # noqa: E731
    alone = npa.maxsim_scores([qs[3]], [ds[2]], **kw)[0]
    batch = npa.maxsim_scores(qs, ds, pairs=[[0], [4, 1], [], [3, 2, 0], [1], [2, 2], [4]], **kw)[3]
    full = npa.maxsim_scores(qs, ds, **kw)[3]
    tq, td = [torch.from_numpy(x).cuda() for x in qs], [torch.from_numpy(x).cuda() for x in ds]
    dev = npa.maxsim_scores(tq, td, pairs=[[2], [], [], [1, 2], [], [], []], **kw)[3]
    torch.cuda.synchronize()
    want = u32(first(alone))[0]
    assert u32(first(batch))[1] == want and u32(first(full))[2] == want and u32(first(dev).cpu().numpy())[1] == want
    if precision == 0:
        for o, k in ((batch, 1), (full, 2), ((dev[0].cpu().numpy(), dev[1].cpu().numpy(), dev[2].cpu().numpy()), 1)):
            assert np.array_equal(u32(o[1][k]), u32(alone[1][0])) and np.array_equal(o[2][k], alone[2][0])
        assert u32(npa.maxsim_scores([qs[3]], [ds[2]])[0])[0] == want          # without the match outputs


@pytest.mark.parametrize("dim", (20, 128, 130, 1024))
def test_matches(dim):
    g = np.random.default_rng(300 + dim)
    q = [M.unit_rows(g, n, dim) for n in (33, 64)]
    d = [M.unit_rows(g, n, dim) for n in (129, 40, 100, 1030)]
    if dim == 1024:   # random rows are ambiguous in 0.3-0.9 % of cases here: plant a near-copy of every query token
        for x in d:
            allq = np.concatenate(q)[: x.shape[0]]
            noisy = allq + 0.05 * M.unit_rows(g, allq.shape[0], dim)
            x[: allq.shape[0]] = noisy / np.linalg.norm(noisy, axis=1, keepdims=True)
    d[1][:] = d[1][7]                      # one token repeated: the lowest index
    d[2][99] = np.nan                      # a NaN row is ignored
    q[0][4] = np.inf                       # every similarity of this token is non-finite: adds 0, reports -1
    out = npa.maxsim_scores(q, d, return_matches=True)
    rows = unchecked = 0
    for i in range(len(q)):
        sc, sims, pos = out[i]
        for j in range(len(d)):
            r = M.pair(q[i], d[j], "f32")
            tot = np.float32(0)
            for x in sims[j]:
                tot = np.float32(tot + x)
            assert u32(tot) == u32(sc[j]) and abs(float(sc[j]) - r["score"]) <= r["bound"]
            assert np.all(np.abs(sims[j] - r["best"]) <= r["bmax"]) and np.array_equal(pos[j] >= 0, r["has"])
            for t in np.nonzero(r["has"])[0]:
                s = np.where(np.isfinite(r["sims"][t]), r["sims"][t], -np.inf)
                b = int(np.argmax(s))
                clear = np.all((s[b] - s > r["tb"][t][b] + r["tb"][t]) | (np.arange(s.size) == b))
                rows += 1
                if j == 1:
                    assert pos[j][t] == 0
                elif clear:
                    assert pos[j][t] == b
                else:
                    unchecked += 1
            if j == 2:
                assert not np.any(pos[j] == 99)
        if i == 0:
            assert np.all(pos[:, 4] == -1) and np.all(sims[:, 4] == 0)
    print(f"dim {dim}: {unchecked} of {rows} rows ambiguous")
    assert unchecked <= (0 if dim == 1024 else 0.005 * rows)      # pairs_restate.AMBIGUOUS_CAP


@pytest.mark.parametrize("name,over,status,word", M.REFUSALS, ids=[r[0] for r in M.REFUSALS])
def test_refusals(name, over, status, word):
    rc, msg, untouched = M.refused_call(api.lib(), over)
    assert rc == status and word in msg and untouched, (rc, msg)
