"""np_hip_maxsim_batch_f16 (np_maxsim_f16.hip) against the float64 reference of tests/maxsim_restate.py on the f16 values widened
to f32: an f16 product has a 22-bit significand and is exact in f32, so pair(q, d, "bf16_rows") -- MFMA step 16, gamma_DIMP A
(1 + 2^-10) per similarity and the per-pair sum term -- is the reference and the bound; no tolerance is measured."""
import numpy as np
import pytest

import maxsim_restate as M
from test_gpu_maxsim_batch import DOC_LENS, LISTS, LQ, u32

from maxsim import maxsim_f16 as F16

pytestmark = pytest.mark.gpu
MODE = "bf16_rows"


def f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16)


def wide(xs):
    return [x.astype(np.float32) for x in xs]


def run(q, d, device=False, **kw):
    """maxsim_scores_f16: numpy float16 through the host entry, or torch.float16 tensors through the device entry."""
    if not device:
        return F16.maxsim_scores_f16(q, d, **kw)
    import torch
    out = F16.maxsim_scores_f16([torch.from_numpy(x).cuda() for x in q], [torch.from_numpy(x).cuda() for x in d], **kw)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("dim", (1, 20, 63, 64, 65, 128, 130, 1024))
def test_shape_grid(dim):
    """Chunk edges (63, 64, 65), the element-load path (dim % 8 != 0), two resident chunks (128) and the double buffer (130, 1024)."""
    g = np.random.default_rng(100 + dim)
    q, d = [f16(M.unit_rows(g, n, dim)) for n in LQ], [f16(M.unit_rows(g, n, dim)) for n in DOC_LENS]
    listed, full = run(q, d, pairs=LISTS), run(q, d)
    worst = 0.0
    for i in range(len(q)):
        assert full[i].shape == (len(d),)
        ref = [M.pair(q[i].astype(np.float32), x.astype(np.float32), MODE) for x in d]
        for got, j in list(zip(listed[i], LISTS[i])) + list(zip(full[i], range(len(d)))):
            err = abs(float(got) - ref[j]["score"])
            worst = max(worst, err / max(ref[j]["bound"], 1e-300))
            assert err <= ref[j]["bound"], (i, j, err, ref[j]["bound"])
        assert np.array_equal(u32(listed[i]), u32(full[i][LISTS[i]]))          # the two forms agree bit for bit
    print(f"dim {dim}: max |err| / bound {worst:.3f}")


def test_shared_workgroups():
    """test_gpu_maxsim_batch.test_shared_workgroups' shape through the device entry: 4 documents and (all pairs) 8 queries per
    workgroup, a 700-token document among short ones, a 3-tile query in 4 slots.  dim 72 = two resident chunks."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256       # else the plan splits these calls further
    g, dim = np.random.default_rng(11), 72
    d = [f16(M.unit_rows(g, n, dim)) for n in np.r_[g.choice([0, 1, 31, 33, 20], 513), 700][g.permutation(514)]]
    q = [f16(M.unit_rows(g, n, dim)) for n in g.integers(1, 33, 33)]
    qlong = [f16(M.unit_rows(g, n, dim)) for n in (70, 5, 32, 33, 96, 1, 64, 17)]
    lists = [g.integers(0, 514, 260) for _ in qlong]
    full, listed = run(q, d, device=True), run(qlong, d, device=True, pairs=lists)
    same = run(q, d, device=True, pairs=[np.arange(514)] * 33)
    for got, qs, ids in ((full, q, [np.arange(514)] * 33), (listed, qlong, lists)):
        score, bound = M.batch(wide(qs), wide(d), MODE)
        for i in range(len(qs)):
            err = np.abs(got[i].astype(np.float64) - score[i][ids[i]])
            print(f"q{i}: max |err| / bound {np.max(err / np.maximum(bound[i][ids[i]], 1e-300)):.3f}")
            assert np.all(err <= bound[i][ids[i]])
    assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(full, same))       # 8 queries and 1 query per workgroup
    for i, k in ((0, 3), (4, 259)):
        assert u32(run([qlong[i]], [d[lists[i][k]]], device=True)[0])[0] == u32(listed[i])[k]


@pytest.mark.parametrize("dim", (20, 128, 130))
def test_matches(dim):
    """test_gpu_maxsim_batch.test_matches' inputs rounded to f16.  The reference alone leaves each of these seeds with 0
    ambiguous rows of 384 (computed on the CPU before the first GPU run): under the 0.5 % cap, no near-copies needed."""
    g = np.random.default_rng(300 + dim)
    q = [M.unit_rows(g, n, dim) for n in (33, 64)]
    d = [M.unit_rows(g, n, dim) for n in (129, 40, 100, 1030)]
    d[1][:] = d[1][7]                      # one token repeated: the lowest index
    d[2][99] = np.nan                      # a NaN row is ignored
    q[0][4] = np.inf                       # every similarity of this token is non-finite: adds 0, reports -1
    q, d = [f16(x) for x in q], [f16(x) for x in d]
    out = run(q, d, return_matches=True)
    rows = unchecked = 0
    for i in range(len(q)):
        sc, sims, pos = out[i]
        for j in range(len(d)):
            r = M.pair(q[i].astype(np.float32), d[j].astype(np.float32), MODE)
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
            assert j != 2 or not np.any(pos[j] == 99)
        assert i or (np.all(pos[:, 4] == -1) and np.all(sims[:, 4] == 0))
    print(f"dim {dim}: {unchecked} of {rows} rows ambiguous")
    assert unchecked <= 0.005 * rows      # pairs_restate.AMBIGUOUS_CAP: a condition on the inputs, not a measurement


def test_subnormal_elements():
    """One 33-token query whose every element is an f16 subnormal (unit rows times 2^-15: |x| < 2^-14), ordinary documents.
    Rows are used as given: the f64 product of the stored values, within the bound."""
    g, dim = np.random.default_rng(64), 64
    q = f16(M.unit_rows(g, 33, dim) * np.float32(2.0 ** -15))
    assert np.all(np.abs(q.astype(np.float32)) < 2.0 ** -14) and np.count_nonzero(q) > 0.9 * q.size
    d = [f16(M.unit_rows(g, n, dim)) for n in (33, 129)]
    got = run([q], d)[0]
    for j, x in enumerate(d):
        r = M.pair(q.astype(np.float32), x.astype(np.float32), MODE)
        print(f"d{j}: score {float(got[j]):.6e} ref {r['score']:.6e} |err| / bound {abs(float(got[j]) - r['score']) / r['bound']:.3f}")
        assert r["score"] > 0 and abs(float(got[j]) - r["score"]) <= r["bound"]
