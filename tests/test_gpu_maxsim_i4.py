"""np_hip_quantize_rows_i4 and np_hip_maxsim_batch_i4 (np_quant.hip, np_maxsim_i4.hip) against tests/maxsim_i4_restate.py and
maxsim_i8_restate.pair on the unpacked nibbles, bit for bit: words, scales, scores, matches.  Only the end-to-end test has a
bound, derived in its docstring."""
import numpy as np
import pytest

import maxsim_i4_restate as Q
import maxsim_i8_restate as R
import maxsim_restate as M
from exact_restate import U, bf16
from test_gpu_maxsim_batch import DOC_LENS, LISTS, LQ, u32

import next_plaid_amd as npa
from maxsim import maxsim_i4 as I4

pytestmark = pytest.mark.gpu


def codes_scales(g, n, dim):
    return g.integers(-128, 128, (n, dim)).astype(np.int8), g.uniform(0.001, 2.0, n).astype(np.float32)


def words_scales(g, n, dim):
    """Random words, the pad nibbles of the last one included, and scales."""
    return g.integers(0, 1 << 32, (n, (dim + 7) // 8), dtype=np.uint64).astype(np.uint32), g.uniform(0.001, 2.0, n).astype(np.float32)


def score(q, d, device=False, **kw):
    """maxsim_scores_i4 of [(rows, scales)] lists: numpy through the host entry, or torch tensors through the device entry."""
    if device:
        import torch
        q = [tuple(torch.from_numpy(a).cuda() for a in x) for x in q]
        d = [(torch.from_numpy(x[0].view(np.int32)).cuda(), torch.from_numpy(x[1]).cuda()) for x in d]
    out = I4.maxsim_scores_i4([x[0] for x in q], [x[1] for x in q], [x[0] for x in d], [x[1] for x in d], **kw)
    return [tuple(a.cpu().numpy() for a in o) if isinstance(o, tuple) else o.cpu().numpy() for o in out] if device else out


def ref_pair(q, d, dim):
    return R.pair(*q, Q.unpack(d[0], dim), d[1])


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("dim", (1, 7, 8, 9, 33, 127, 128, 129, 1024))
def test_quantiser(dim, dtype):
    """Four workgroups, the last one partial; rows: random at mixed magnitudes, all zero, +0.0 and -0.0 mixed, half-way values
    k + 0.5 under an extreme of -7 (inv is exactly 1: ties to even show), a NaN and an inf."""
    import torch
    g = np.random.default_rng(dim)
    x = (g.standard_normal((13, dim)) * g.uniform(1e-3, 50, (13, 1))).astype(np.float32)
    x[3] = 0
    x[5] = np.where(g.integers(0, 2, dim) > 0, 0.0, -0.0)
    x[9] = g.integers(-7, 7, dim) + 0.5
    x[9, 0] = -7
    x[7, dim // 2], x[11, dim - 1] = np.nan, np.inf
    if dtype == "bf16":
        x = bf16(x)
    words, scales = Q.quantize4(x, 8 if dtype == "bf16" else 4)
    assert not scales[[3, 5]].any() and np.isnan(scales[[7, 11]]).all() and scales[9] == 1 and not words[[3, 5, 7, 11]].any()
    assert np.abs(Q.unpack(words, dim)).max() == 7 and (dim % 8 == 0 or not np.any(words[:, -1] >> np.uint32(4 * (dim % 8))))   # pad nibbles are 0
    t = torch.from_numpy(x).cuda()
    got = [tuple(a.cpu().numpy() for a in I4.quantize_rows_i4(t.to(torch.bfloat16) if dtype == "bf16" else t))]   # the device entry
    for w, s in got + ([I4.quantize_rows_i4(x)] if dtype == "f32" else []):                                       # ... and the host entry
        assert np.array_equal(w.view(np.uint32), words) and np.array_equal(u32(s), u32(scales))


@pytest.mark.parametrize("dim", (1, 7, 8, 9, 31, 32, 40, 63, 64, 65, 127, 128, 129, 200, 1024))
def test_scores(dim):
    g = np.random.default_rng(500 + dim)
    q, d = [codes_scales(g, n, dim) for n in LQ], [words_scales(g, n, dim) for n in DOC_LENS]
    if dim == 1024:
        q[1][0][:], d[4][0][:] = -128, 0x88888888                         # every code -8: the accumulator is 2^24, the largest there is
    listed, full = score(q, d, pairs=LISTS), score(q, d)
    for i in range(len(q)):
        ref = np.array([ref_pair(q[i], d[j], dim)[0] for j in range(len(d))], np.float32)
        assert np.array_equal(u32(full[i]), u32(ref)) and np.array_equal(u32(listed[i]), u32(ref[LISTS[i]]))


@pytest.mark.parametrize("dim", (17, 128, 1024))
def test_matches(dim):
    g = np.random.default_rng(700 + dim)
    q, d = [codes_scales(g, n, dim) for n in (33, 64)], [words_scales(g, n, dim) for n in (129, 40, 100, 1030)]
    d[1][0][:], d[1][1][:] = d[1][0][7], d[1][1][7]       # one token repeated: the lowest index
    d[2][1][99] = np.nan                                  # a NaN scale: never reported
    q[0][1][4] = np.inf                                   # every similarity of this token is non-finite: 0.0 / -1
    back = [3, 2, 1, 0]
    for out, order in ((score(q, d, return_matches=True), range(4)), (score(q, d, device=True, return_matches=True, pairs=[back] * 2), back)):
        for i in range(len(q)):
            for k, j in enumerate(order):
                sc, sims, pos = ref_pair(q[i], d[j], dim)
                assert u32(out[i][0])[k] == u32(sc) and np.array_equal(u32(out[i][1][k]), u32(sims)) and np.array_equal(out[i][2][k], pos)
                assert not (j == 1 and np.any(pos[pos >= 0] != 0)) and not (j == 2 and np.any(pos == 99))
            assert i or (np.all(out[i][2][:, 4] == -1) and np.all(out[i][1][:, 4] == 0))


@pytest.mark.parametrize("dim,qlong", ((72, (70, 5, 32, 33, 96, 1, 64, 17)), (200, (70, 5, 32, 33, 96, 1, 64, 17)), (264, (170, 5, 32, 33, 200, 1, 64, 17))))
def test_shared_workgroups(dim, qlong):
    """test_gpu_maxsim_b1.test_shared_workgroups' shape: 4 documents and (all pairs) 8 queries per workgroup, a 700-token document
    among short ones.  dim 72 = one chunk, slots staged once; dim 200 = two chunks, W = 25: dword loads, two slot buffers (the
    listed call: its longest query has 96 tokens, nqt = 3, so maxsim_plan takes NQT = 4); dim 264 = three chunks and ONE buffer
    in both calls: maxsim_plan takes NQT = 8 when G * nqt > 4, which the listed call reaches with G = 1 and nqt = ceil(200 / 32)
    = 7 on any device, and the all-pairs call with nqt = 1 and G = 8, kept because ceil(33 / 8) * ceil(514 / 4) = 645
    workgroups are at least twice the compute units (hence the assertion)."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256
    g = np.random.default_rng(11 + dim)
    d = [words_scales(g, n, dim) for n in np.r_[g.choice([0, 1, 31, 33, 20], 513), 700][g.permutation(514)]]
    q = [codes_scales(g, n, dim) for n in g.integers(1, 33, 33)]
    qlong = [codes_scales(g, n, dim) for n in qlong]
    lists = [g.integers(0, 514, 260) for _ in qlong]
    du = [(Q.unpack(x[0], dim), x[1]) for x in d]         # the reference's documents, unpacked once
    ref = lambda qs, ids: [np.array([R.pair(*x, *du[j])[0] for j in ids[i]], np.float32) for i, x in enumerate(qs)]   # noqa: E731
    for qs, pairs, want in ((q, None, ref(q, [range(514)] * 33)), (qlong, lists, ref(qlong, lists))):
        for dev in (False, True):
            got = score(qs, d, device=dev, pairs=pairs)
            assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("dim", (128, 200))
def test_same_bits_as_the_int8_kernel(dim):
    """The nibbles unpacked to int8 through maxsim_scores (np_maxsim.hip MODE 3) give the same score bits."""
    g = np.random.default_rng(900 + dim)
    q, d = [codes_scales(g, n, dim) for n in LQ], [words_scales(g, n, dim) for n in DOC_LENS]
    i8 = npa.maxsim_scores([x[0] for x in q], [Q.unpack(x[0], dim) for x in d], query_scales=[x[1] for x in q], document_scales=[x[1] for x in d])
    assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(score(q, d), i8))


def test_end_to_end_against_float64():
    """int8 queries (quantize_rows) and int4 documents (quantize_rows_i4) of unit rows at dim 128 against the f64 MaxSim of the
    original rows.  Bound, nothing measured, propagated as test_gpu_maxsim_i8's: a dequantised element differs from x by at most
    e = (a / C) / 2 * (1 + eta), a = max|x|, C = 7 or 127; one similarity by sum_d(|q_d| e_d + |d_d| e_q + e_q e_d), plus the two
    f32 multiplications by the scales, 2.0001 u of the dequantised similarity; a pair as maxsim_restate.pair sums its bound.
    eta from the quantiser's three roundings: code * scale - x = (code - p) scale + (p scale - x) with p = fl(x *
    fl(C / a)) and scale = fl(a / C) <= (a / C)(1 + u): the first term is at most scale / 2, the second |x| ((1 + u)^3 - 1) <=
    a * 3.0001 u = (a / C) / 2 * 6.0002 C u, so eta = (6.0002 C + 1.01) u: 44 u for C = 7, 764 u for C = 127."""
    g, dim = np.random.default_rng(1900), 128
    q, d = [M.unit_rows(g, n, dim) for n in (33, 5)], [M.unit_rows(g, n, dim) for n in (129, 40, 1030)]
    out = score([npa.quantize_rows(x) for x in q], [I4.quantize_rows_i4(x) for x in d])
    for i, x in enumerate(q):
        for j, y in enumerate(d):
            x64, y64 = x.astype(np.float64), y.astype(np.float64)
            eq, ed = np.abs(x64).max(1) / 127 / 2 * (1 + 764 * U), np.abs(y64).max(1) / 7 / 2 * (1 + 44 * U)
            sims = x64 @ y64.T
            tb = np.abs(x64).sum(1)[:, None] * ed[None, :] + eq[:, None] * np.abs(y64).sum(1)[None, :] + dim * eq[:, None] * ed[None, :]
            tb += 2.0001 * U * (np.abs(sims) + tb)
            best, bmax = sims.max(1), tb.max(1)
            bound = bmax.sum() + (x.shape[0] - 1) * U * (np.abs(best) + bmax).sum()
            print(f"q{i} d{j}: |err| {abs(float(out[i][j]) - best.sum()):.3e} bound {bound:.3e}")
            assert abs(float(out[i][j]) - best.sum()) <= bound
