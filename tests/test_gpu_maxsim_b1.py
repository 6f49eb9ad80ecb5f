"""np_hip_pack_rows_b1 and np_hip_maxsim_batch_b1 (np_quant.hip, np_maxsim_b1.hip) against tests/maxsim_b1_restate.py and
maxsim_i8_restate.pair on the unpacked bits, bit for bit: words, scales, scores, matches."""
import numpy as np
import pytest

import maxsim_b1_restate as B
import maxsim_i8_restate as R
from exact_restate import bf16
from test_gpu_maxsim_batch import DOC_LENS, LISTS, LQ, u32

import next_plaid_amd as npa
from maxsim import maxsim_b1 as B1

pytestmark = pytest.mark.gpu


def codes_scales(g, n, dim):
    return g.integers(-128, 128, (n, dim)).astype(np.int8), g.uniform(0.001, 2.0, n).astype(np.float32)


def bits_scales(g, n, dim):
    """Random words, the pad bits of the last one included, and scales."""
    return g.integers(0, 1 << 32, (n, (dim + 31) // 32), dtype=np.uint64).astype(np.uint32), g.uniform(0.001, 2.0, n).astype(np.float32)


def score(q, d, device=False, **kw):
    """maxsim_scores_b1 of [(rows, scales)] lists: numpy through the host entry, or torch tensors through the device entry."""
    if device:
        import torch
        q = [tuple(torch.from_numpy(a).cuda() for a in x) for x in q]
        d = [(torch.from_numpy(x[0].view(np.int32)).cuda(), torch.from_numpy(x[1]).cuda()) for x in d]
    out = B1.maxsim_scores_b1([x[0] for x in q], [x[1] for x in q], [x[0] for x in d], [x[1] for x in d], **kw)
    return [tuple(a.cpu().numpy() for a in o) if isinstance(o, tuple) else o.cpu().numpy() for o in out] if device else out


def ref_pair(q, d, dim):
    return R.pair(*q, B.unpack(d[0], dim), d[1])


@pytest.mark.parametrize("dtype", ("f32", "bf16"))
@pytest.mark.parametrize("dim", (1, 31, 32, 33, 127, 128, 129, 1024))
def test_packer(dim, dtype):
    """Four workgroups, the last one partial; rows: random at mixed magnitudes, all zero, +0.0 and -0.0 mixed, a NaN, an inf."""
    import torch
    g = np.random.default_rng(dim)
    x = (g.standard_normal((13, dim)) * g.uniform(1e-3, 50, (13, 1))).astype(np.float32)
    x[3] = 0
    x[5] = np.where(g.integers(0, 2, dim) > 0, 0.0, -0.0)
    x[7, dim // 2], x[11, dim - 1] = np.nan, np.inf
    if dtype == "bf16":
        x = bf16(x)
    bits, scales = B.pack(x, 8 if dtype == "bf16" else 4)
    assert scales[3] == 0 and scales[5] == 0 and np.isnan(scales[[7, 11]]).all() and np.all(B.unpack(bits[[3, 5]], dim) == 1)
    assert dim % 32 == 0 or not np.any(bits[:, -1] >> np.uint32(dim % 32))                                    # pad bits are 0
    t = torch.from_numpy(x).cuda()
    got = [tuple(a.cpu().numpy() for a in B1.pack_rows_b1(t.to(torch.bfloat16) if dtype == "bf16" else t))]   # the device entry
    for w, s in got + ([B1.pack_rows_b1(x)] if dtype == "f32" else []):                                       # ... and the host entry
        assert np.array_equal(w.view(np.uint32), bits) and np.array_equal(u32(s), u32(scales))


@pytest.mark.parametrize("dim", (1, 31, 32, 33, 127, 128, 129, 160, 1024))
def test_scores(dim):
    g = np.random.default_rng(500 + dim)
    q, d = [codes_scales(g, n, dim) for n in LQ], [bits_scales(g, n, dim) for n in DOC_LENS]
    if dim == 1024:
        q[1][0][:], d[4][0][:] = -128, 0                                  # dot = 2^17, the largest there is
    listed, full = score(q, d, pairs=LISTS), score(q, d)
    for i in range(len(q)):
        ref = np.array([ref_pair(q[i], d[j], dim)[0] for j in range(len(d))], np.float32)
        assert np.array_equal(u32(full[i]), u32(ref)) and np.array_equal(u32(listed[i]), u32(ref[LISTS[i]]))


@pytest.mark.parametrize("dim", (17, 128, 1024))
def test_matches(dim):
    g = np.random.default_rng(700 + dim)
    q, d = [codes_scales(g, n, dim) for n in (33, 64)], [bits_scales(g, n, dim) for n in (129, 40, 100, 1030)]
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


@pytest.mark.parametrize("dim", (72, 200))
def test_shared_workgroups(dim):
    """test_gpu_maxsim_i8.test_shared_workgroups_and_resident_slots' shape: 4 documents and (all pairs) 8 queries per workgroup,
    a 700-token document among short ones; dim 72 = one chunk, slots staged once; dim 200 = two chunks, W = 7: dword loads."""
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count <= 256
    g = np.random.default_rng(11 + dim)
    d = [bits_scales(g, n, dim) for n in np.r_[g.choice([0, 1, 31, 33, 20], 513), 700][g.permutation(514)]]
    q = [codes_scales(g, n, dim) for n in g.integers(1, 33, 33)]
    qlong = [codes_scales(g, n, dim) for n in (70, 5, 32, 33, 96, 1, 64, 17)]
    lists = [g.integers(0, 514, 260) for _ in qlong]
    du = [(B.unpack(x[0], dim), x[1]) for x in d]         # the reference's documents, unpacked once
    ref = lambda qs, ids: [np.array([R.pair(*x, *du[j])[0] for j in ids[i]], np.float32) for i, x in enumerate(qs)]   # noqa: E731
    for qs, pairs, want in ((q, None, ref(q, [range(514)] * 33)), (qlong, lists, ref(qlong, lists))):
        for dev in (False, True):
            got = score(qs, d, device=dev, pairs=pairs)
            assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(got, want))


@pytest.mark.parametrize("dim", (128, 200))
def test_same_bits_as_the_int8_kernel(dim):
    """The bits unpacked to +-1 int8 through maxsim_scores (np_maxsim.hip MODE 3) give the same score bits."""
    g = np.random.default_rng(900 + dim)
    q, d = [codes_scales(g, n, dim) for n in LQ], [bits_scales(g, n, dim) for n in DOC_LENS]
    i8 = npa.maxsim_scores([x[0] for x in q], [B.unpack(x[0], dim) for x in d], query_scales=[x[1] for x in q], document_scales=[x[1] for x in d])
    assert all(np.array_equal(u32(a), u32(b)) for a, b in zip(score(q, d), i8))
