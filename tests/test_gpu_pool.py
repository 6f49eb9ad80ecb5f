"""np_hip_pool_documents (token pooling on the GPU, np_pool.hip) against the numpy f64 restatement of the reference
(tests/pool_restate.py): linkage rows as u64 bit patterns, labels, pooled rows as u32 bit patterns, all EQUAL on every
document -- no tolerance, no document left out.  Needs a real MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pool_restate as R
from helpers import ROOT

import next_plaid_amd as npa
from next_plaid_amd import api

pytestmark = pytest.mark.gpu

CUTS = {0: "reference", 1: "distance"}


def _compare(docs, factor, prot, cut_order, **kw):
    """Pools `docs` in one call and holds every document against the restatement.  Returns the pooled documents."""
    pooled, labels, det = api.pool_document_embeddings(docs, factor, prot, cut=CUTS[cut_order], return_labels=True,
                                                       return_details=True, **kw)
    assert len(pooled) == len(labels) == len(det["linkage"]) == len(docs)
    want_len = [R.pooled_length(d.shape[0], factor, prot) for d in docs]
    assert [p.shape[0] for p in pooled] == want_len == api.pooled_lengths([d.shape[0] for d in docs], factor, prot).tolist()
    rep = det["report"]
    assert rep["n_docs"] == len(docs) and rep["tokens_in"] == sum(d.shape[0] for d in docs)
    assert rep["tokens_out"] == sum(want_len)
    assert rep["n_pooled"] == sum(w != d.shape[0] for w, d in zip(want_len, docs))
    for i, x in enumerate(docs):
        o, l, Z = R.pool_document(x, factor, prot, cut_order)
        tag = f"doc {i} ({x.shape[0]} tokens, dim {x.shape[1]}, factor {factor}, protected {prot}, cut {cut_order})"
        if Z is None:
            assert det["linkage"][i] is None, tag
        else:
            got = det["linkage"][i]
            assert got.shape == Z.shape, tag
            bad = np.nonzero(got.view(np.uint64) != Z.view(np.uint64))
            assert bad[0].size == 0, f"{tag}: {bad[0].size} linkage values differ, first at row {bad[0][0]}: " \
                                     f"{got[bad[0][0]]} vs {Z[bad[0][0]]}"
        assert np.array_equal(labels[i], l), f"{tag}: labels differ"
        assert pooled[i].shape == o.shape and np.array_equal(pooled[i].view(np.uint32), o.view(np.uint32)), f"{tag}: rows differ"
    return pooled


def test_every_length_to_300_and_1030():
    docs = R.gpu_corpus(128)
    assert [d.shape[0] for d in docs] == list(range(301)) + [1030]
    for cut in (0, 1):
        _compare(docs, 2, 1, cut)


@pytest.mark.parametrize("dim", [48, 96, 100])
def test_other_dims(dim):
    docs = R.gpu_corpus(dim, stride=13)
    _compare(docs, 2, 1, 0)
    _compare(docs, 3, 1, 1)


@pytest.mark.parametrize("factor", [1, 2, 3, 4, 1000])
@pytest.mark.parametrize("prot", [0, 1, 2])
def test_factors_and_protected_tokens(factor, prot):
    tied = R.cache_sensitive_document()
    docs = R.gpu_corpus(64, stride=7, long_doc=False) + [np.pad(tied, ((0, 0), (0, 64 - tied.shape[1])))]
    for cut in (0, 1):
        pooled = _compare(docs, factor, prot, cut)
        if factor == 1:
            assert all(np.array_equal(p, d) for p, d in zip(pooled, docs))


def test_ties_and_the_cache_rule():
    """Duplicate rows, zero rows, rows that differ in the last bit, lattices of equal distances, and the document on which
    a fresh nearest-neighbour search and the reference's cache part ways: the GPU follows the cache."""
    rng = np.random.default_rng(77)
    tied = [R.tied_document(rng, int(n), 32) for n in rng.integers(6, 150, 30)]
    lattice = [R.lattice_document(rng, int(n), 16) for n in rng.integers(4, 150, 30)]
    lattice += [np.zeros((9, 16), np.float32), np.ones((17, 16), np.float32)]
    x = R.cache_sensitive_document()
    for cut in (0, 1):
        _compare(tied, 2, 1, cut)            # one call takes documents of one dim
        _compare(lattice, 2, 1, cut)
        _compare([x], 2, 1, cut)
    fresh = R.pool_document(x, 2, use_cache=False)
    got, lab = api.pool_document_embeddings([x], 2, return_labels=True)
    assert not np.array_equal(lab[0], fresh[1]) and not np.array_equal(got[0], fresh[0])


def test_the_longest_supported_document():
    x = R.corpus_document(128, 2049)           # 2048 tokens go to the clustering: the limit
    _compare([x], 2, 1, 0)
    _compare([x], 4, 1, 1)


def test_alone_in_a_batch_and_under_forced_chunks():
    docs = R.gpu_corpus(96, stride=17)
    whole, wl = api.pool_document_embeddings(docs, 2, return_labels=True)
    for cd in (1, 3):
        part, pl = api.pool_document_embeddings(docs, 2, return_labels=True, chunk_docs=cd)
        for a, b, c, d in zip(whole, part, wl, pl):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(c, d)
    for i in (3, 9, len(docs) - 1):
        alone, al = api.pool_document_embeddings([docs[i]], 2, return_labels=True)
        assert np.array_equal(alone[0].view(np.uint32), whole[i].view(np.uint32)) and np.array_equal(al[0], wl[i])
    rev = api.pool_document_embeddings(docs[::-1], 2)[::-1]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, rev))
    # where the matrix lives (LDS or the scratch) does not show in the result
    env = dict(os.environ, NP_POOL_LDS_MAX="0", PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "next-plaid_amd"), os.path.join(ROOT, "tests")]))
    code = ("import numpy as np, pool_restate as R\nfrom next_plaid_amd import api\n"
            "docs = R.gpu_corpus(96, stride=17)\n"
            "out = api.pool_document_embeddings(docs, 2)\n"
            "import sys; sys.stdout.buffer.write(np.concatenate(out, 0).tobytes())\n")
    raw = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, timeout=600)
    assert raw.returncode == 0, raw.stderr[-2000:]
    assert raw.stdout == np.concatenate(whole, 0).tobytes()


CPP = r"""
#include <cstdio>
#include <vector>
#include "next_plaid.hpp"
int main(int argc, char** argv) {
  if (argc < 6) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  int64_t hdr[2];
  if (!f || std::fread(hdr, 8, 2, f) != 2) return 2;
  next_plaid::Documents d;
  d.dim = (size_t)hdr[1];
  d.doc_lengths.resize((size_t)hdr[0]);
  if (std::fread(d.doc_lengths.data(), 8, d.doc_lengths.size(), f) != d.doc_lengths.size()) return 2;
  int64_t rows = 0;
  for (int64_t v : d.doc_lengths) rows += v;
  std::vector<float> emb((size_t)rows * d.dim);
  if (std::fread(emb.data(), 4, emb.size(), f) != emb.size()) return 2;
  std::fclose(f);
  d.embeddings = emb.data();
  try {
    auto lens = next_plaid::pooled_lengths(d.doc_lengths, std::atoi(argv[3]), std::atoi(argv[4]));
    auto r = next_plaid::pool_document_embeddings(d, std::atoi(argv[3]), std::atoi(argv[4]),
                                                  std::atoi(argv[5]) ? next_plaid::PoolCut::Distance : next_plaid::PoolCut::Reference,
                                                  0, true);
    if (lens != r.doc_lengths) return 3;
    FILE* o = std::fopen(argv[2], "wb");
    std::fwrite(r.doc_lengths.data(), 8, r.doc_lengths.size(), o);
    std::fwrite(r.labels.data(), 4, r.labels.size(), o);
    std::fwrite(r.embeddings.data(), 4, r.embeddings.size(), o);
    std::fclose(o);
  } catch (const next_plaid::Error& e) {
    std::fprintf(stderr, "next-plaid error %d: %s\n", (int)e.kind, e.what());
    return 1;
  }
  return 0;
}
"""


def test_cpp_mirror_gives_the_same_bytes(tmp_path):
    src = tmp_path / "pool_cli.cpp"
    src.write_text(CPP)
    exe = tmp_path / "pool_cli"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), str(src), "-o", str(exe),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    docs = R.gpu_corpus(128, stride=19)
    lens = np.array([d.shape[0] for d in docs], np.int64)
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(docs), 128], np.int64).tobytes() + lens.tobytes() + np.concatenate(docs, 0).tobytes())
    for cut in (0, 1):
        subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "2", "1", str(cut)])
        pooled, labels = api.pool_document_embeddings(docs, 2, cut=CUTS[cut], return_labels=True)
        want = (np.array([p.shape[0] for p in pooled], np.int64).tobytes() + np.concatenate(labels).tobytes()
                + np.concatenate(pooled, 0).tobytes())
        assert open(tmp_path / "out.bin", "rb").read() == want
    nan = tmp_path / "nan.bin"
    bad = np.full((4, 128), np.nan, np.float32)
    nan.write_bytes(np.array([1, 128], np.int64).tobytes() + np.array([4], np.int64).tobytes() + bad.tobytes())
    pr = subprocess.run([str(exe), str(nan), str(tmp_path / "o2.bin"), "2", "1", "0"], capture_output=True, text=True)
    assert pr.returncode == 1 and "error 8" in pr.stderr and "non-finite" in pr.stderr


def test_pooled_documents_build_a_searchable_index(tmp_path):
    rng = np.random.default_rng(5)
    docs = [R.clustered_document(rng, int(n), 128) for n in rng.integers(8, 90, 600)]
    pooled = npa.pool_document_embeddings(docs, 2)
    plen = npa.pooled_lengths([d.shape[0] for d in docs], 2)
    assert [p.shape[0] for p in pooled] == plen.tolist() and plen.sum() < sum(d.shape[0] for d in docs) * 0.56
    hx = npa.MmapIndex.create_with_kmeans(pooled, str(tmp_path / "ix"), npa.IndexConfig(nbits=4, seed=3))
    assert hx.num_documents() == len(docs) and hx.num_embeddings() == int(plen.sum())
    p = npa.SearchParameters(top_k=5, n_ivf_probe=8, n_full_scores=256)
    ids = [7, 123, 410]
    res = hx.search_batch([docs[i][1:17] for i in ids], p)
    for r, i in zip(res, ids):
        assert len(r.passage_ids) == 5 and np.all(np.isfinite(r.scores))
        assert i in r.passage_ids.tolist()
    hx.close()


def test_refused_inputs():
    x = R.corpus_document(32, 40)
    bad = x.copy()
    bad[17, 5] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        api.pool_document_embeddings([x, bad], 2)
    bad[17, 5] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        api.pool_document_embeddings([bad], 2)
    with pytest.raises(ValueError):
        api.pool_document_embeddings([x], 2, cut="scipy")
    with pytest.raises(ValueError):
        api.pool_document_embeddings([x], 2, protected_tokens=-1)
    with pytest.raises(npa.ShapeError):
        api.pool_document_embeddings([x, x[:, :16]], 2)
    long_doc = np.zeros((2050, 8), np.float32)
    long_doc[:, 0] = 1.0
    with pytest.raises(npa.ShapeError, match="2048"):
        api.pool_document_embeddings([x[:, :8], long_doc], 2)
    # ... but only where it would be clustered: factor 1 copies it through
    out = api.pool_document_embeddings([long_doc], 1)
    assert np.array_equal(out[0], long_doc)
    assert api.pool_document_embeddings([], 2) == []
    o = api.np_pool_opts(2, 1, 0, 0, 0)
    lens = np.array([40], np.int64)
    small = np.zeros((3, 32), np.float32)
    rc = api.lib().np_hip_pool_documents(0, api._ptr(x), api._ptr(lens), 1, 32, api.C.byref(o), api._ptr(small), 3, None, None,
                                         None, None)
    assert rc == 8 and "rows" in api.last_error()
