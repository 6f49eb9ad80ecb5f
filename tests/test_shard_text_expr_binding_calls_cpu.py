"""Which entry a batch of keyword queries reaches through dist.CShardedSearcher and what stands behind its structs -- without
a device and without the library.  A fake stands in for api._lib and records, per entry, the values behind every pointer; the
outputs are CPU tensors, so the fake's rows come back as results.  Checked: a text.TextExpr in the batch sends the whole batch
to the sharded _expr entry (flat queries lifted to chains), a flat batch keeps its entry, the filtered and the hybrid forms,
the communicator and the stream among the arguments, that full_grammar is off unless asked for, and that the grouped search
still refuses a tree by name.  (next_plaid.hpp mirrors neither the sharded nor the device-pointer keyword calls: there is
nothing of it to run here.)"""
import contextlib
import ctypes as C
import types

import numpy as np
import pytest

from next_plaid_amd import api, dist, text as T

from test_text_expr_binding_calls_cpu import FakeLib as HostFake, rd

P, AND, OR, NOT = T.NP_TEXT_NODE_PHRASE, T.NP_TEXT_NODE_AND, T.NP_TEXT_NODE_OR, T.NP_TEXT_NODE_NOT
STREAM = 0x5EED


def addr(p):
    return p if isinstance(p, int) or p is None else p.value


class FakeLib(HostFake):
    """the sharded entries beside the host ones of tests/test_text_expr_binding_calls_cpu.py"""

    def _sharded(self, name, rec, h, c, tq, B, k, sid, soff, hoff, n_sub, qsub, ids, sc, cnt, stream):
        self.calls.append((name, dict(comm=addr(c), B=B, top_k=k, queries=rec(tq, B), n_sub=n_sub, stream=addr(stream),
                                      h_off=None if hoff is None else rd(hoff, np.int64, n_sub + 1).tolist(),
                                      qmap=None if qsub is None else rd(qsub, np.int32, B).tolist())))
        return self._rows(ids, sc, cnt, B, k)

    def np_hip_text_search_sharded(self, *a):
        return self._sharded("np_hip_text_search_sharded", self._flat, *a)

    def np_hip_text_search_sharded_expr(self, h, c, tq, *a):
        assert isinstance(tq[0], api.np_text_expr)
        return self._sharded("np_hip_text_search_sharded_expr", self._trees, h, c, tq, *a)

    def _filtered(self, name, rec, h, c, tq, B, k, f, nf, qf, ids, sc, cnt, stream):
        self.calls.append((name, dict(comm=addr(c), B=B, top_k=k, queries=rec(tq, B), n_filters=nf, stream=addr(stream),
                                      qmap=rd(qf, np.int32, B).tolist())))
        return self._rows(ids, sc, cnt, B, k)

    def np_hip_text_search_sharded_filtered(self, *a):
        return self._filtered("np_hip_text_search_sharded_filtered", self._flat, *a)

    def np_hip_text_search_sharded_expr_filtered(self, *a):
        return self._filtered("np_hip_text_search_sharded_expr_filtered", self._trees, *a)

    def _hybrid_sharded(self, name, rec, h, c, dq, do, hoff, B, dim, p, tq, fk, alpha, fusion, sid, soff, hsoff, n_sub, qsub, f, nf, qf,
                        ids, sc, cnt, stream):
        self.calls.append((name, dict(comm=addr(c), B=B, dim=dim, top_k=p._obj.top_k, fetch_k=fk, alpha=alpha, fusion=fusion,
                                      queries=rec(tq, B), n_sub=n_sub, filters=f is not None, n_filters=nf, stream=addr(stream),
                                      tok_off=rd(hoff, np.int32, B + 1).tolist(), d_tok_off=rd(do, np.int32, B + 1).tolist(),
                                      qf=None if qf is None else rd(qf, np.int32, B).tolist())))
        return self._rows(ids, sc, cnt, B, p._obj.top_k)

    def np_hip_search_hybrid_sharded(self, *a):
        return self._hybrid_sharded("np_hip_search_hybrid_sharded", self._flat, *a)

    def np_hip_search_hybrid_sharded_expr(self, *a):
        return self._hybrid_sharded("np_hip_search_hybrid_sharded_expr", self._trees, *a)


class CpuTorch:
    """torch with its stream context a no-op: the tensors of a call live on the CPU, where the fake can write them"""

    def __init__(self):
        import torch
        self._t = torch
        self.cuda = types.SimpleNamespace(stream=lambda s: contextlib.nullcontext())

    def __getattr__(self, name):
        return getattr(self._t, name)


@pytest.fixture
def cs(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(api, "_lib", f)
    x = object.__new__(api.MmapIndex)
    x._h, x._info = C.c_void_p(1), api.np_info()
    x._info.embedding_dim, x._info.num_documents = 4, 50
    x.text = T.TextIndexData.from_texts(["ab abc b", "abd ca", "b ca cab", "zz"])
    s = dist.CShardedSearcher.__new__(dist.CShardedSearcher)
    s.torch = CpuTorch()
    s.index, s.device = x, s.torch.device("cpu")
    s.comm = types.SimpleNamespace(_h=C.c_void_p(2), status=lambda: (-1, 0))
    s.stream = types.SimpleNamespace(cuda_stream=STREAM, synchronize=lambda: None)
    s.fake = f
    yield s
    x._h = None   # (nothing to close: the handle never was the library's)


def test_a_mixed_batch_reaches_the_sharded_expr_entry_with_flat_queries_lifted(cs):
    v = cs.index.text.vocab
    tree = T.compile_text_expr('(ab OR "b ca") NOT ab*', cs.index.text)
    flat = T.TextQuery.from_phrases([[v["b"]], [v["ca"], v["cab"]], [-1]], T.NP_TEXT_OR)
    some = np.array([1, 2])
    res = cs.text_search([flat, tree, "", "ca b"], 3, subsets=[None, some, None, some])
    (name, c), = cs.fake.calls
    assert name == "np_hip_text_search_sharded_expr" and c["B"] == 3 and c["top_k"] == 3      # the empty query is not sent
    assert c["comm"] == 2 and c["stream"] == STREAM
    assert c["n_sub"] == 1 and c["qmap"] == [-1, 0, 0] and c["h_off"] == [0, 2]
    assert c["queries"][0] == dict(terms=[v["b"], v["ca"], v["cab"], -1], off=[0, 1, 3, 4], hi=[0, 0, 0],
                                   nodes=[[P, 0, 0], [P, 1, 0], [OR, 0, 1], [P, 2, 0], [OR, 2, 3]])
    assert c["queries"][1] == dict(terms=[v["ab"], v["b"], v["ca"], v["ab"]], off=[0, 1, 3, 4], hi=[0, 0, v["abd"] + 1],
                                   nodes=[[P, 0, 0], [P, 1, 0], [OR, 0, 1], [P, 2, 0], [NOT, 2, 3]])
    assert c["queries"][2] == dict(terms=[v["ca"], v["b"]], off=[0, 1, 2], hi=[0, 0], nodes=[[P, 0, 0], [P, 1, 0], [AND, 0, 1]])
    assert [r.passage_ids.tolist() for r in res] == [[100], [101], [], [102]] and res[3].query_id == 3
    assert res[1].scores.tolist() == [2.5]


def test_a_flat_batch_keeps_its_entry_and_full_grammar_is_off_by_default(cs):
    v = cs.index.text.vocab
    cs.text_search(["ab b", T.TextQuery.from_phrases([[0]], T.NP_TEXT_OR)], 2)
    (name, c), = cs.fake.calls
    assert name == "np_hip_text_search_sharded" and [q["mode"] for q in c["queries"]] == [T.NP_TEXT_AND, T.NP_TEXT_OR]
    assert c["queries"][0]["terms"] == [v["ab"], v["b"]] and c["n_sub"] == 0 and c["qmap"] is None
    for text, what in (("ab NOT b", "NOT"), ("ab*", r"\*"), ("(ab)", "parentheses")):
        with pytest.raises(T.TextQueryError, match=what):
            cs.text_search([text], 2)
        with pytest.raises(T.TextQueryError, match=what):
            cs.search_hybrid([np.zeros((2, 4), np.float32)], [text], api.SearchParameters(top_k=2))
    assert len(cs.fake.calls) == 1
    cs.text_search(["ab NOT b", "ab*", "(ab)", "ab b"], 2, full_grammar=True)
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_text_search_sharded_expr" and c["B"] == 4
    assert c["queries"][0]["nodes"] == [[P, 0, 0], [P, 1, 0], [NOT, 0, 1]] and c["queries"][1]["hi"] == [v["abd"] + 1]
    assert c["queries"][2]["nodes"] == [[P, 0, 0]] and c["queries"][3]["nodes"] == [[P, 0, 0], [P, 1, 0], [AND, 0, 1]]
    # full_grammar over flat text alone still goes to the tree entry: the strings were compiled into trees
    cs.text_search(["ab b"], 2, full_grammar=True)
    assert cs.fake.calls[-1][0] == "np_hip_text_search_sharded_expr"
    # an empty prefix range crosses as the unknown token
    cs.text_search(["q*"], 2, full_grammar=True)
    assert cs.fake.calls[-1][1]["queries"][0] == dict(terms=[-1], off=[0, 1], hi=[0], nodes=[[P, 0, 0]])


def test_the_device_form_takes_trees_as_they_are(cs):
    tree = T.compile_text_expr("ab NOT b", cs.index.text)
    flat = T.TextQuery.from_phrases([[1], [2]], T.NP_TEXT_AND)
    rc, out = cs.text_search_device([flat, tree], 5)
    name, c = cs.fake.calls[-1]
    assert rc == 0 and name == "np_hip_text_search_sharded_expr" and c["B"] == 2 and c["top_k"] == 5 and c["n_sub"] == 0
    assert c["queries"][0] == dict(terms=[1, 2], off=[0, 1, 2], hi=[0, 0], nodes=[[P, 0, 0], [P, 1, 0], [AND, 0, 1]])
    assert out[0].shape == (2, 5) and out[0][1, 0].item() == 101 and out[2].tolist() == [1, 1]
    rc, out = cs.text_search_device([flat, flat], 5)
    assert cs.fake.calls[-1][0] == "np_hip_text_search_sharded"


def test_the_filtered_and_the_hybrid_forms(cs, monkeypatch):
    monkeypatch.setattr(api.MmapIndex, "_filters", lambda self, filters, n: (api._CFilters([]), np.zeros(n, np.int32)))
    tree = T.compile_text_expr("ab NOT b", cs.index.text)
    cs.text_search([tree, "ca"], 2, filters=[("z = ?", [1])] * 2)
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_text_search_sharded_expr_filtered" and c["B"] == 2 and c["qmap"] == [0, 0]
    assert len(c["queries"][1]["nodes"]) == 1 and c["comm"] == 2 and c["stream"] == STREAM
    cs.text_search(["ab", "ca"], 2, filters=[("z = ?", [1])] * 2)
    assert cs.fake.calls[-1][0] == "np_hip_text_search_sharded_filtered"
    qs = [np.zeros((2, 4), np.float32), np.ones((3, 4), np.float32)]
    p = api.SearchParameters(top_k=2)
    cs.search_hybrid(qs, ["ab", ""], p)
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_search_hybrid_sharded" and c["fetch_k"] == 6 and c["queries"][1]["terms"] == [-1]
    res = cs.search_hybrid(qs, [tree, ""], p, alpha=0.5, fusion="rrf", fetch_k=9)
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_search_hybrid_sharded_expr"
    assert (c["B"], c["dim"], c["top_k"], c["fetch_k"], c["alpha"], c["fusion"]) == (2, 4, 2, 9, 0.5, 0)
    assert c["tok_off"] == [0, 2, 5] and c["d_tok_off"] == [0, 2, 5] and c["comm"] == 2 and c["stream"] == STREAM
    assert c["queries"][0]["nodes"] == [[P, 0, 0], [P, 1, 0], [NOT, 0, 1]] and not c["filters"] and c["qf"] is None
    assert c["queries"][1] == dict(terms=[-1], off=[0, 1], hi=[0], nodes=[[P, 0, 0]])      # the empty query matches nothing
    assert [r.passage_ids.tolist() for r in res] == [[100], [101]]
    cs.search_hybrid(qs, ["ab OR (b NOT ca)", "ab*"], p, full_grammar=True, subsets=[np.array([3, 4]), None])
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_search_hybrid_sharded_expr" and c["n_sub"] == 1 and len(c["queries"][0]["nodes"]) == 5
    cs.search_hybrid(qs, [tree, "ab"], p, filters=[("z = ?", [1])] * 2)
    name, c = cs.fake.calls[-1]
    assert name == "np_hip_search_hybrid_sharded_expr" and c["filters"] and c["qf"] == [0, 0]
    # the grouped searches still have no _expr form, and the message names only them
    with pytest.raises(ValueError, match="no _expr form yet") as e:
        cs.index.search_hybrid_grouped(qs, [tree, "ab"], p)
    assert "grouped" in str(e.value) and "sharded" not in str(e.value) and "device-pointer" not in str(e.value)
