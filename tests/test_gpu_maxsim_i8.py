"""np_hip_quantize_rows_i8 and np_hip_maxsim_batch_i8 (np_quant.hip, np_maxsim.hip MODE 3) against tests/maxsim_i8_restate.py,
bit for bit: codes, scales, scores, matches.  Only the end-to-end test has a bound, derived in its docstring."""
import numpy as np
import pytest

import maxsim_i8_restate as R
import maxsim_restate as M
from exact_restate import U, bf16
from test_gpu_maxsim_batch import DOC_LENS, LISTS, LQ, u32

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu


def codes_scales(g, n, dim):
    return g.integers(-128, 128, (n, dim)).astype(np.int8), g.uniform(0.001, 2.0, n).astype(np.float32)


def score(q, d, device=False, **kw):
    """maxsim_scores of [(codes, scales)] lists: numpy through the host entry, or torch tensors through the device entry."""
    if device:
        import torch
        q, d = ([tuple(torch.from_numpy(a).cuda() for a in x) for x in xs] for xs in (q, d))
    out = npa.maxsim_scores([x[0] for x in q], [x[0] for x in d], query_scales=[x[1] for x in q], document_scales=[x[1] for x in d], **kw)
    return [tuple(a.cpu().numpy() for a in o) if isinstance(o, tuple) else o.cpu().numpy() for o in out] if device else out


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("dim", (1, 15, 16, 17, 127, 128, 129, 1024))
def test_quantiser(dim, dtype):
    """Four workgroups, the last one partial; rows: random, all zero, half-way values k + 0.5 under an extreme of -127 (inv is
    exactly 1: ties to even show), a NaN and an inf."""
    import torch
    g = np.random.default_rng(dim)
    x = (g.standard_normal((13, dim)) * g.uniform(1e-3, 50, (13, 1))).astype(np.float32)
    x[3] = 0
    x[5] = g.integers(-127, 127, dim) + 0.5
    x[5, 0] = -127
    x[7, dim // 2], x[11, dim - 1] = np.nan, np.inf
    if dtype == "bf16":
        x = bf16(x)
    codes, scales = R.quantize(x)
    assert scales[3] == 0 and np.isnan(scales[[7, 11]]).all() and scales[5] == 1 and codes[5, 0] == -127
    t = torch.from_numpy(x).cuda()
    got = [tuple(a.cpu().numpy() for a in npa.quantize_rows(t.to(torch.bfloat16) if dtype == "bf16" else t))]      # the device entry
    for c, s in got + ([npa.quantize_rows(x)] if dtype == "f32" else []):                                         # ... and the host entry
        assert c.dtype == np.int8 and np.array_equal(c, codes) and np.array_equal(u32(s), u32(scales))


@pytest.mark.parametrize("dim", (1, 16, 17, 127, 128, 129, 130, 256, 1024))
def test_scores(dim):
    g = np.random.default_rng(500 + dim)
    q, d = [codes_scales(g, n, dim) for n in LQ], [codes_scales(g, n, dim) for n in DOC_LENS]
    if dim == 1024:
        q[1][0][:], d[4][0][:] = -128, -128                               # dot = 2^24, the largest there is
    listed, full = score(q, d, pairs=LISTS), score(q, d)
    for i in range(len(q)):
        ref = np.array([R.pair(*q[i], *d[j])[0] for j in range(len(d))], np.float32)
        assert np.array_equal(u32(full[i]), u32(ref)) and np.array_equal(u32(listed[i]), u32(ref[LISTS[i]]))


@pytest.mark.parametrize("dim", (17, 128, 1024))
def test_matches(dim):
    g = np.random.default_rng(700 + dim)
    q, d = [codes_scales(g, n, dim) for n in (33, 64)], [codes_scales(g, n, dim) for n in (129, 40, 100, 1030)]
    d[1][0][:], d[1][1][:] = d[1][0][7], d[1][1][7]       # one token repeated: the lowest index
    d[2][1][99] = np.nan                                  # a NaN scale: never reported
    q[0][1][4] = np.inf                                   # every similarity of this token is non-finite: 0.0 / -1
    back = [3, 2, 1, 0]
    for out, order in ((score(q, d, return_matches=True), range(4)), (score(q, d, device=True, return_matches=True, pairs=[back] * 2), back)):
        for i in range(len(q)):
            for k, j in enumerate(order):
                sc, sims, pos = R.pair(*q[i], *d[j])
                assert u32(out[i][0])[k] == u32(sc) and np.array_equal(u32(out[i][1][k]), u32(sims)) and np.array_equal(out[i][2][k], pos)
                assert not (j == 1 and np.any(pos[pos >= 0] != 0)) and not (j == 2 and np.any(pos == 99))
            assert i or (np.all(out[i][2][:, 4] == -1) and np.all(out[i][1][:, 4] == 0))


def test_shared_workgroups_and_resident_slots():
    """test_gpu_maxsim_batch.test_shared_workgroups' shape: the plan keeps 4 documents and (all pairs) 8 queries per workgroup,
    a 700-token document among short ones, dim 72 = one chunk, so the slots are staged once.  Every score bit-equal."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256
    g, dim = np.random.default_rng(11), 72
    d = [codes_scales(g, n, dim) for n in np.r_[g.choice([0, 1, 31, 33, 20], 513), 700][g.permutation(514)]]
    q = [codes_scales(g, n, dim) for n in g.integers(1, 33, 33)]
    qlong = [codes_scales(g, n, dim) for n in (70, 5, 32, 33, 96, 1, 64, 17)]
    lists = [g.integers(0, 514, 260) for _ in qlong]
    ref = lambda qs, ids: [np.array([R.pair(*x, *d[j])[0] for j in ids[i]], np.float32) for i, x in enumerate(qs)]   # noqa: E731
    for qs, pairs, want in ((q, None, ref(q, [range(514)] * 33)), (qlong, lists, ref(qlong, lists))):
        for dev in (False, True):
            got = score(qs, d, device=dev, pairs=pairs)
            assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("dim", (128, 1024))
def test_end_to_end_against_float64(dim):
    """Quantised unit rows against the f64 MaxSim of the original rows.  Bound, nothing measured: a dequantised element differs
    from x by at most e = scale / 2 * (1 + 2^-22); one similarity by sum_d(|q_d| e_d + |d_d| e_q + e_q e_d), plus the two f32
    multiplications by the scales, 2.0001 u of the dequantised similarity (at most |ref| + that sum); a pair as
    maxsim_restate.pair sums its bound."""
    g = np.random.default_rng(900 + dim)
    q, d = [M.unit_rows(g, n, dim) for n in (33, 5)], [M.unit_rows(g, n, dim) for n in (129, 40, 1030)]
    out = score([npa.quantize_rows(x) for x in q], [npa.quantize_rows(x) for x in d])
    for i, x in enumerate(q):
        for j, y in enumerate(d):
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            eq, ed = (np.abs(z).max(1) / 127 / 2 * (1 + 2.0 ** -22) for z in (x64, y64))
            sims = x64 @ y64.T
            tb = np.abs(x64).sum(1)[:, None] * ed[None, :] + eq[:, None] * np.abs(y64).sum(1)[None, :] + dim * eq[:, None] * ed[None, :]
            tb += 2.0001 * U * (np.abs(sims) + tb)
            best, bmax = sims.max(1), tb.max(1)
            bound = bmax.sum() + (x.shape[0] - 1) * U * (np.abs(best) + bmax).sum()
            print(f"dim {dim} q{i} d{j}: |err| {abs(float(out[i][j]) - best.sum()):.3e} bound {bound:.3e}")
            assert abs(float(out[i][j]) - best.sum()) <= bound
