"""The expansion mode of the index update (find_outliers: km_norm_kernel, one nearest_step, ol_flag_kernel,
ol_recheck_kernel; then k-means, encode with encode_norm_kernel, update_cluster_threshold) held to the answers that
tests/update_limit_shapes.py states, with no tolerance: the outlier count and the exact number of rechecked tokens, the new
centroid rows byte for byte, the threshold bit for bit, and every file of the directory against the restated sequence.

tests/test_update_limits_cpu.py shows on the restatement that the cases bite.  Needs a real MI355X.
"""
import os
import shutil

import numpy as np
import pytest

import update_limit_shapes as S
import update_restate as U

import next_plaid_amd as npa

pytestmark = pytest.mark.gpu

A_CASES = S.outlier_cases()
B_CASES = S.norm_cases()


def _write(path, cen, nbits, thr, n_base, seed=1):
    a = S.base_index(cen, nbits, n_base, seed)
    npa.write_index_dir(str(path), a["centroids"], a["bucket_weights"], a["doc_lengths"], a["codes"], a["residuals"], nbits,
                        bucket_cutoffs=a["bucket_cutoffs"], cluster_threshold=0.0 if thr is None else float(thr))
    tp = os.path.join(str(path), "cluster_threshold.npy")
    if thr is None:
        os.remove(tp)
    else:
        assert np.load(tp).tobytes() == np.array([thr], np.float32).tobytes()
    return int(a["doc_lengths"].size)


def _config(mppc=256):
    return npa.UpdateConfig(buffer_size=0, start_from_scratch=0, kmeans_niters=S.KMEANS_NITERS, max_points_per_centroid=mppc,
                            seed=S.SEED)


def _same_state(a, b, what):
    sa, sb = U.dir_state(str(a)), U.dir_state(str(b))
    assert sa.keys() == sb.keys(), what
    for f in sa:
        assert sa[f] == sb[f], f"{what}: {f}"


def _expand_and_check(a, b, case, via_handle=False):
    """One expansion of directory a with the case's documents against the restated sequence on its copy b."""
    cen = np.load(os.path.join(a, "centroids.npy"))
    thr = np.load(os.path.join(a, "cluster_threshold.npy"))[0]
    assert cen.tobytes() == case.centroids.tobytes() and thr.tobytes() == np.float32(case.thr).tobytes()
    before = open(os.path.join(a, "centroids.npy"), "rb").read()
    n_old = U._j(os.path.join(a, "metadata.json"))["num_documents"]
    cfg = _config(case.mppc)
    assert U.mode(b, len(case.docs), 0, 0) == "expansion"
    if via_handle:
        hx = npa.MmapIndex.load(a)
        ids, rep = hx.update(case.docs, cfg), hx.last_update
        hx.close()
    else:
        ids, rep = npa.update_index_dir(a, case.docs, cfg)
    assert rep["mode"] == "expansion" and ids.tolist() == list(range(n_old, n_old + len(case.docs)))
    out = case.outliers
    print(f"{case.name}: tokens {case.flat.shape[0]}, outliers {rep['n_outliers']} (restated {out.size}), rechecked "
          f"{rep['n_rechecked']} (stated {case.n_rechecked}), new centroids {rep['n_new_centroids']}")
    assert rep["n_outliers"] == out.size, case.name
    assert rep["n_rechecked"] == case.n_rechecked, case.name
    newc = np.load(os.path.join(a, "centroids.npy"))
    if out.size:
        k_up = U.k_update(out.size, case.mppc)
        kc = npa.compute_kmeans([case.flat[i][None] for i in out],
                                npa.IndexConfig(nbits=case.nbits, kmeans_niters=S.KMEANS_NITERS, max_points_per_centroid=case.mppc,
                                                seed=S.SEED), num_partitions=k_up)
        assert rep["n_new_centroids"] == kc.shape[0] == k_up == newc.shape[0] - cen.shape[0]
        assert newc[:cen.shape[0]].tobytes() == cen.tobytes() and newc[cen.shape[0]:].tobytes() == kc.tobytes()
        np.save(os.path.join(b, "centroids.npy"), newc)
    else:
        assert rep["n_new_centroids"] == 0 and open(os.path.join(a, "centroids.npy"), "rb").read() == before
    U.update_index(b, case.docs, 50_000, True)
    _same_state(a, b, case.name)
    return rep


@pytest.mark.parametrize("case", A_CASES, ids=lambda c: c.name)
def test_outlier_search(tmp_path, case):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write(a, case.centroids, case.nbits, case.thr, case.n_base, case.base_seed)
    shutil.copytree(a, b)
    rep = _expand_and_check(a, b, case)
    if case.flat.shape[0] == 0:                       # nothing to search or encode: the threshold stays
        assert rep["n_outliers"] == rep["n_rechecked"] == 0
        assert np.load(os.path.join(a, "cluster_threshold.npy"))[0] == case.thr


def test_second_expansion_meets_a_partly_filled_tile(tmp_path):
    """The directory the (33, 64) case leaves has K = 33 + 4: tile 1 holds five centroids (four of them new) and 27 padding
    slots.  The recipes are rebuilt around those centroids and the blended threshold, through a handle this time."""
    first = next(c for c in A_CASES if c.name.startswith("mix-K33-d64"))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _write(a, first.centroids, first.nbits, first.thr, first.n_base, first.base_seed)
    shutil.copytree(a, b)
    _expand_and_check(a, b, first)
    cen = np.load(os.path.join(a, "centroids.npy"))
    thr = np.load(os.path.join(a, "cluster_threshold.npy"))[0]
    assert cen.shape[0] == 37 and thr != first.thr
    second = S.second_case(cen, thr, first.nbits)
    assert second.band().size == 0, "an input condition: no token in (w/2, 2w] of the threshold"
    rep = _expand_and_check(a, b, second, via_handle=True)
    assert rep["n_rechecked"] >= 24 and rep["n_outliers"] > 0


@pytest.mark.parametrize("case", B_CASES, ids=lambda c: c.name)
def test_residual_norms_through_the_threshold(tmp_path, case):
    """Without cluster_threshold.npy the outlier search is skipped and the file written is the 0.75 quantile itself: the
    norm of the one token at the probed position (two for the even n), bit for bit.  With the file present over a
    one-token index, the f32 blend of the old threshold and that quantile."""
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    n_old = _write(a, case.centroids, case.nbits, case.old_thr, case.n_base)
    shutil.copytree(a, b)
    before = open(os.path.join(a, "centroids.npy"), "rb").read()
    ids, rep = npa.update_index_dir(a, case.docs, _config())
    assert rep["mode"] == "expansion" and ids.tolist() == list(range(n_old, n_old + len(case.docs)))
    assert rep["n_outliers"] == rep["n_rechecked"] == rep["n_new_centroids"] == 0
    assert open(os.path.join(a, "centroids.npy"), "rb").read() == before
    got = np.load(os.path.join(a, "cluster_threshold.npy"))
    q = case.quantile
    if case.old_thr is None:
        want = q
        if len(case.probes) == 1:
            assert want.tobytes() == case.norms[case.probes[0]].tobytes()
    else:
        old_t = U._j(os.path.join(b, "metadata.json"))["num_embeddings"]
        n = case.flat.shape[0]
        assert old_t == 1
        want = (np.float32(case.old_thr) * np.float32(old_t) + q * np.float32(n)) / np.float32(old_t + n)
    print(f"{case.name}: threshold {got[0]!r}, stated {want!r}")
    assert got.dtype == np.float32 and got.shape == (1,) and got.tobytes() == np.float32(want).tobytes(), case.name
    codes = U.update_index(b, case.docs, 50_000, True)
    assert np.array_equal(codes, case.codes)
    _same_state(a, b, case.name)
