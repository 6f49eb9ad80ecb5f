"""tests/update_limit_shapes.py bites: on the numpy restatement alone (no device), every case states what it claims and the
wrong rules it is meant to catch change its answer.  tests/test_gpu_update_limits.py then holds the device to those answers.
"""
import numpy as np
import pytest

import kmeans_restate as R
import update_limit_shapes as S
import update_restate as U

A_CASES = S.outlier_cases()
B_CASES = S.norm_cases()
F32 = np.float32


def _case(prefix):
    return next(c for c in A_CASES if c.name.startswith(prefix))


@pytest.mark.parametrize("case", A_CASES, ids=lambda c: c.name)
def test_recipes_band_and_f32_error(case):
    """Every recipe has the stated membership under find_outliers (f64); no token lies in (w/2, 2w] of thr^2; the f32
    emulation of the first pass stays within w/2 of the f64 distance on every token, so it lists exactly the tokens
    with |d - thr^2| <= w/2."""
    out = np.zeros(case.flat.shape[0], bool)
    out[case.outliers] = True
    known = case.expect >= 0
    bad = np.nonzero(known & (out != (case.expect == 1)))[0]
    assert bad.size == 0, f"{case.name}: token {bad[:5]} ({case.labels[bad[:5]]}) outlier={out[bad[:5]]}, d={case.d64[bad[:5]]}"
    assert sum(d.shape[0] == 0 for d in case.docs) >= 1 or case.name == "single-token"
    band = case.band()
    assert band.size == 0, f"{case.name}: tokens {band[:5]} ({case.labels[band[:5]]}) lie in (w/2, 2w] of thr^2"
    if case.flat.shape[0] == 0:
        return
    d32 = U.min_dist_sq_f32(case.flat, case.centroids)
    err = np.abs(d32.astype(np.float64) - case.d64)
    assert np.all(err <= case.w / 2), f"{case.name}: f32 error {err.max():.3g} against w/2 {case.w[np.argmax(err)] / 2:.3g}"
    listed = np.abs(d32 - F32(case.thr2)) <= case.w.astype(F32)
    assert int(listed.sum()) == case.n_rechecked
    # what the recipes are for
    for label, inside in (("edge", True), ("outside", case.name.startswith("large"))):
        m = case.labels == label
        if m.any():
            assert np.all(listed[m] == inside), f"{case.name}: {label} tokens listed: {listed[m].sum()} of {m.sum()}"


def test_cases_cover_what_they_name():
    names = [c.name for c in A_CASES]
    assert len(set(names)) == len(names)
    for K, dim, *_ in S.GEOMETRIES:
        c = _case(f"mix-K{K}-d{dim}b")
        assert c.centroids.shape == (K, dim) and set(S.RECIPES) <= set(c.labels.tolist())
        assert {0, 1} <= set(np.isin(np.arange(c.flat.shape[0]), c.outliers)[c.labels == "edge"].tolist()), c.name
    assert {c.nbits for c in A_CASES} == {2, 4} and {c.mppc for c in A_CASES} == {1, 256}
    lst = _case("list-")
    edge = np.nonzero(lst.labels == "edge")[0]
    assert edge.size >= 700 and lst.n_rechecked >= 700
    assert all(np.any(edge // 256 == b) for b in range(3)), "the list is fed from three blocks of 256 tokens"
    for n_out, mppc in S.COUNTS:
        assert _case(f"count{n_out}-mppc{mppc}").outliers.size == n_out
    assert _case("single-token").outliers.size == 1 and _case("all-empty").flat.shape[0] == 0
    assert _case("mix-K33-d64").outliers.size > 4       # k_update = 4: the second expansion meets K = 37


@pytest.mark.parametrize("dim", [64, 128])
def test_large_norms_need_the_second_window_term(dim):
    """At centroid norm 25 the f32 first pass alone puts planted tokens on the wrong side although they lie outside the
    crate's window max(thr^2, 1) 1e-5: only the term 4 (Dp + 2) 2^-24 (|x|^2 + max |c|^2) sends them to the recheck."""
    case = _case(f"large-K33-d{dim}")
    planted = case.labels == "outside"
    assert planted.sum() == 400 and np.allclose(np.linalg.norm(case.centroids, axis=1), 25.0, rtol=1e-5)
    d32 = U.min_dist_sq_f32(case.flat, case.centroids)
    truth = np.zeros(planted.size, bool)
    truth[case.outliers] = True
    crate_w = max(case.thr2, 1.0) * 1e-5
    wrong = planted & ((d32 > F32(case.thr2)) != truth) & (np.abs(case.d64 - case.thr2) > crate_w)
    print(f"dim {dim}: {int(wrong.sum())} of 400 planted tokens misplaced by the f32 pass outside the 1e-5 window")
    assert wrong.sum() >= 1
    assert np.all(np.abs(case.d64 - case.thr2)[wrong] <= case.w[wrong] / 2)       # the full window lists them all


def test_a_zero_centroid_slot_would_take_the_origin_tokens():
    case = _case("mix-K33-d64")
    padded = np.concatenate([case.centroids, np.zeros((1, 64), F32)])        # the tile's slot 33 as a centroid
    origin = np.nonzero(case.labels == "origin")[0]
    assert np.isin(origin, case.outliers).all()
    assert not np.isin(origin, U.find_outliers(case.flat, padded, case.thr)).any()
    assert np.any(np.all(case.flat[origin] == 0, axis=1))


def test_ge_flips_the_on_centroid_tokens_at_threshold_zero():
    case = _case("thr0-")
    on = np.nonzero(case.labels == "on")[0]
    d = U.min_dist_sq_precise(case.flat, case.centroids)
    assert case.thr2 == 0.0 and np.all(d[on] == 0) and not np.isin(on, case.outliers).any()
    assert np.all(d[on] >= F32(case.thr2))
    others = np.setdiff1d(np.arange(d.size), on)
    assert np.isin(others, case.outliers).all()


def test_second_expansion_builder_on_stand_in_centroids():
    """second_case() is built on the GPU test's own centroids; here on 33 + 4 unit rows in their place"""
    first = _case("mix-K33-d64")
    cen = np.concatenate([first.centroids, S.unit_centroids(4, 64, 9)])
    c = S.second_case(cen, F32(0.29))
    assert c.band().size == 0 and set(S.RECIPES) <= set(c.labels.tolist())


@pytest.mark.parametrize("case", B_CASES, ids=lambda c: c.name)
def test_the_probe_token_is_the_quantile(case):
    n = case.flat.shape[0]
    norms = case.norms
    assert np.array_equal(np.argsort(np.argsort(norms, kind="stable"), kind="stable"), case.ranks), "norms order as the radii"
    assert np.unique(norms).size == n
    # the encode's choice does not rest on rounding: the best score leads by more than two f32 dot products can be off
    s = np.sort(case.flat.astype(np.float64) @ case.centroids.astype(np.float64).T, axis=1)
    lead = s[:, -1] - s[:, -2]
    bound = 2 * case.flat.shape[1] * 2.0 ** -24 * np.linalg.norm(case.flat, axis=1) * np.linalg.norm(case.centroids, axis=1).max()
    assert np.all(lead > bound), f"{case.name}: a code is decided by {lead.min():.3g}"
    q = case.quantile
    if len(case.probes) == 1:
        p = case.probes[0]
        assert n % 4 == 1 and n >= 2081 and q.tobytes() == norms[p].tobytes()
        k = 3 * (n - 1) // 4
        up = np.nextafter(norms, F32(np.inf))
        for i in range(n):                      # one ulp on token p moves the quantile, on any other token it does not
            v = norms.copy()
            v[i] = up[i]
            assert (np.partition(v, k)[k] != q) == (i == p), (case.name, i)
    else:
        lo, hi = case.probes
        assert np.array_equal(np.sort(case.ranks[[lo, hi]]), [3 * (n - 1) // 4, 3 * (n - 1) // 4 + 1])
        assert q ==F32(F32(norms[lo] * F32(0.25)) + F32(norms[hi] * F32(0.75)))
        for i in (lo, hi):
            v = norms.copy()
            v[i] = v[0]
            assert R.quantile(np.sort(v), 0.75) != q
    # slice 2 given the norms of slice 1 (out_norms without + t0, or a stale buffer)
    v = norms.copy()
    v[S.SLICE:] = norms[:n - S.SLICE]
    moved = R.quantile(np.sort(v), 0.75) != q
    if any(p >= S.SLICE for p in case.probes):
        assert moved, case.name
    # rows read with the storage stride instead of the file's (dim 100 in rows of 128)
    dim = case.flat.shape[1]
    if U.storage_dim(dim) != dim:
        flat = case.flat.reshape(-1)
        sd = U.storage_dim(dim)
        rows = min(n, flat.size // sd)
        strided = np.stack([flat[i * sd:i * sd + dim] for i in range(rows)])
        assert R.quantile(np.sort(U.residual_norms(strided, case.centroids, case.codes[:rows])), 0.75) != q


def test_norm_probes_cover_the_slices():
    names = [c.name for c in B_CASES]
    assert len(set(names)) == len(names)
    for K, dim, nbits in S.NORM_GEOMETRIES:
        got = {c.probes for c in B_CASES if c.name.endswith(f"-K{K}-d{dim}b{nbits}") and c.name.startswith("p")}
        assert got == {(0,), (31,), (32,), (2047,), (2048,), (S.N_ODD - 1,)}
    assert S.SLICE == 2048 and S.N_ODD - S.SLICE == 33
    even = next(c for c in B_CASES if c.name.startswith("even"))
    assert even.flat.shape[0] % 2 == 0 and even.probes == (2047, 2048)
    blend = next(c for c in B_CASES if c.name.startswith("blend"))
    assert blend.n_base == 1 and blend.old_thr == 4.0
    # the blend moves with the quantile: one ulp on the probe token's norm changes the f32 expression
    n = blend.flat.shape[0]
    o, q = F32(blend.old_thr), blend.quantile
    mix = lambda qq: (o * F32(1) + qq * F32(n)) / F32(1 + n)      # noqa: E731
    assert mix(q) != mix(np.nextafter(q, F32(np.inf))) or mix(q) != mix(np.nextafter(q, F32(0)))
