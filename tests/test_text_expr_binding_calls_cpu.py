"""Which entry a batch of keyword queries reaches and what stands behind its structs -- without a device and without the
library.  A fake stands in for api._lib and records, per entry, the values behind every pointer; the C++ mirror runs against
recording stubs in tests/cpp/text_expr_binding_check.cpp.  Checked: a text.TextExpr in the batch sends the whole batch to
the _expr entry (flat queries lifted to chains), a flat batch keeps its entry, the phrases, prefix ranges and nodes of
np_text_expr, the filtered and the hybrid forms, and that full_grammar is off unless asked for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from next_plaid_amd import api, text as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, AND, OR, NOT = T.NP_TEXT_NODE_PHRASE, T.NP_TEXT_NODE_AND, T.NP_TEXT_NODE_OR, T.NP_TEXT_NODE_NOT


def rd(ptr, dtype, n):
    if int(n) == 0:
        return np.zeros(0, dtype)
    addr = ptr if isinstance(ptr, int) else ptr.value
    assert addr, "a NULL pointer where entries are read"
    return np.frombuffer((C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(addr), dtype).copy()


class FakeLib:
    def __init__(self):
        self.calls = []

    def np_hip_last_error(self):
        return b"Invalid argument: the fake said so"

    def _rows(self, ids, sc, cnt, B, k):
        for i in range(B):
            C.cast(cnt, C.POINTER(C.c_int32))[i] = 1
            C.cast(ids, C.POINTER(C.c_int64))[i * k] = 100 + i
            C.cast(sc, C.POINTER(C.c_float))[i * k] = 1.5 + i
        return 0

    @staticmethod
    def _flat(arr, B):
        return [dict(terms=rd(q.terms, np.int32, rd(q.phrase_offsets, np.int32, q.n_phrases + 1)[-1]).tolist(),
                     off=rd(q.phrase_offsets, np.int32, q.n_phrases + 1).tolist(), mode=q.mode) for q in arr[:B]]

    @staticmethod
    def _trees(arr, B):
        out = []
        for q in arr[:B]:
            off = rd(q.phrase_offsets, np.int32, q.n_phrases + 1)
            out.append(dict(terms=rd(q.terms, np.int32, off[-1]).tolist(), off=off.tolist(),
                            hi=rd(q.prefix_hi, np.int32, q.n_phrases).tolist(),
                            nodes=rd(q.nodes, np.int32, 3 * q.n_nodes).reshape(-1, 3).tolist()))
        return out

    def np_hip_text_search(self, h, tq, B, k, sid, soff, n_sub, qmap, ids, sc, cnt, st):
        self.calls.append(("np_hip_text_search", dict(B=B, top_k=k, queries=self._flat(tq, B), n_sub=n_sub)))
        return self._rows(ids, sc, cnt, B, k)

    def np_hip_text_search_expr(self, h, tq, B, k, sid, soff, n_sub, qmap, ids, sc, cnt, st):
        assert isinstance(tq[0], api.np_text_expr)
        self.calls.append(("np_hip_text_search_expr", dict(B=B, top_k=k, queries=self._trees(tq, B), n_sub=n_sub,
                                                           qmap=None if qmap is None else rd(qmap, np.int32, B).tolist())))
        return self._rows(ids, sc, cnt, B, k)

    def np_hip_text_search_filtered(self, h, tq, B, k, f, nf, qmap, ids, sc, cnt, st):
        self.calls.append(("np_hip_text_search_filtered", dict(B=B, queries=self._flat(tq, B), n_filters=nf)))
        return self._rows(ids, sc, cnt, B, k)

    def np_hip_text_search_expr_filtered(self, h, tq, B, k, f, nf, qmap, ids, sc, cnt, st):
        self.calls.append(("np_hip_text_search_expr_filtered", dict(B=B, queries=self._trees(tq, B), n_filters=nf,
                                                                    qmap=rd(qmap, np.int32, B).tolist())))
        return self._rows(ids, sc, cnt, B, k)

    def _hybrid(self, name, rec, h, q, off, B, dim, p, tq, fk, alpha, fusion, sid, soff, n_sub, qmap, f, nf, ids, sc, cnt, st):
        self.calls.append((name, dict(B=B, dim=dim, top_k=p._obj.top_k, fetch_k=fk, alpha=alpha, fusion=fusion, queries=rec(tq, B),
                                      n_sub=n_sub, filters=f is not None)))
        return self._rows(ids, sc, cnt, B, p._obj.top_k)

    def np_hip_search_hybrid(self, *a):
        return self._hybrid("np_hip_search_hybrid", self._flat, *a)

    def np_hip_search_hybrid_expr(self, *a):
        return self._hybrid("np_hip_search_hybrid_expr", self._trees, *a)


@pytest.fixture
def ix(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(api, "_lib", f)
    x = object.__new__(api.MmapIndex)
    x._h, x._info = C.c_void_p(1), api.np_info()
    x._info.embedding_dim, x._info.num_documents = 4, 50
    x.text = T.TextIndexData.from_texts(["ab abc b", "abd ca", "b ca cab", "zz"])
    x.fake = f
    yield x
    x._h = None   # (nothing to close: the handle never was the library's)


def test_a_mixed_batch_reaches_the_expr_entry_with_flat_queries_lifted(ix):
    v = ix.text.vocab
    tree = T.compile_text_expr('(ab OR "b ca") NOT ab*', ix.text)
    flat = T.TextQuery.from_phrases([[v["b"]], [v["ca"], v["cab"]], [-1]], T.NP_TEXT_OR)
    some = np.array([1, 2])
    res = ix.text_search([flat, tree, "", "ca b"], 3, subsets=[None, some, None, some])
    (name, c), = ix.fake.calls
    assert name == "np_hip_text_search_expr" and c["B"] == 3 and c["top_k"] == 3      # the empty query is not sent
    assert c["n_sub"] == 1 and c["qmap"] == [-1, 0, 0]
    assert c["queries"][0] == dict(terms=[v["b"], v["ca"], v["cab"], -1], off=[0, 1, 3, 4], hi=[0, 0, 0],
                                   nodes=[[P, 0, 0], [P, 1, 0], [OR, 0, 1], [P, 2, 0], [OR, 2, 3]])
    assert c["queries"][1] == dict(terms=[v["ab"], v["b"], v["ca"], v["ab"]], off=[0, 1, 3, 4], hi=[0, 0, v["abd"] + 1],
                                   nodes=[[P, 0, 0], [P, 1, 0], [OR, 0, 1], [P, 2, 0], [NOT, 2, 3]])
    assert c["queries"][2] == dict(terms=[v["ca"], v["b"]], off=[0, 1, 2], hi=[0, 0], nodes=[[P, 0, 0], [P, 1, 0], [AND, 0, 1]])
    assert [r.passage_ids.tolist() for r in res] == [[100], [101], [], [102]] and res[3].query_id == 3
    assert res[1].scores.tolist() == [2.5]


def test_a_flat_batch_keeps_its_entry_and_full_grammar_is_off_by_default(ix):
    v = ix.text.vocab
    ix.text_search(["ab b", T.TextQuery.from_phrases([[0]], T.NP_TEXT_OR)], 2)
    (name, c), = ix.fake.calls
    assert name == "np_hip_text_search" and [q["mode"] for q in c["queries"]] == [T.NP_TEXT_AND, T.NP_TEXT_OR]
    assert c["queries"][0]["terms"] == [v["ab"], v["b"]]
    for text, what in (("ab NOT b", "NOT"), ("ab*", r"\*"), ("(ab)", "parentheses")):
        with pytest.raises(T.TextQueryError, match=what):
            ix.text_search([text], 2)
        with pytest.raises(T.TextQueryError, match=what):
            ix.search_hybrid([np.zeros((2, 4), np.float32)], [text], api.SearchParameters(top_k=2))
    assert len(ix.fake.calls) == 1
    ix.text_search(["ab NOT b", "ab*", "(ab)", "ab b"], 2, full_grammar=True)
    name, c = ix.fake.calls[-1]
    assert name == "np_hip_text_search_expr" and c["B"] == 4
    assert c["queries"][0]["nodes"] == [[P, 0, 0], [P, 1, 0], [NOT, 0, 1]] and c["queries"][1]["hi"] == [v["abd"] + 1]
    assert c["queries"][2]["nodes"] == [[P, 0, 0]] and c["queries"][3]["nodes"] == [[P, 0, 0], [P, 1, 0], [AND, 0, 1]]
    # an empty prefix range crosses as the unknown token
    ix.text_search(["q*"], 2, full_grammar=True)
    assert ix.fake.calls[-1][1]["queries"][0] == dict(terms=[-1], off=[0, 1], hi=[0], nodes=[[P, 0, 0]])


def test_the_filtered_and_the_hybrid_forms(ix, monkeypatch):
    monkeypatch.setattr(api.MmapIndex, "_filters", lambda self, filters, n: (api._CFilters([]), np.zeros(n, np.int32)))
    tree = T.compile_text_expr("ab NOT b", ix.text)
    ix.text_search([tree, "ca"], 2, filters=[("z = ?", [1])] * 2)
    name, c = ix.fake.calls[-1]
    assert name == "np_hip_text_search_expr_filtered" and c["B"] == 2 and c["qmap"] == [0, 0] and len(c["queries"][1]["nodes"]) == 1
    ix.text_search(["ab", "ca"], 2, filters=[("z = ?", [1])] * 2)
    assert ix.fake.calls[-1][0] == "np_hip_text_search_filtered"
    qs = [np.zeros((2, 4), np.float32), np.ones((3, 4), np.float32)]
    p = api.SearchParameters(top_k=2)
    ix.search_hybrid(qs, ["ab", ""], p)
    name, c = ix.fake.calls[-1]
    assert name == "np_hip_search_hybrid" and c["fetch_k"] == 6 and c["queries"][1]["terms"] == [-1]
    ix.search_hybrid(qs, [tree, ""], p, alpha=0.5, fusion="rrf", fetch_k=9)
    name, c = ix.fake.calls[-1]
    assert name == "np_hip_search_hybrid_expr" and (c["B"], c["dim"], c["top_k"], c["fetch_k"], c["alpha"], c["fusion"]) == (2, 4, 2, 9, 0.5, 0)
    assert c["queries"][0]["nodes"] == [[P, 0, 0], [P, 1, 0], [NOT, 0, 1]]
    assert c["queries"][1] == dict(terms=[-1], off=[0, 1], hi=[0], nodes=[[P, 0, 0]])      # the empty query matches nothing
    ix.search_hybrid(qs, ["ab OR (b NOT ca)", "ab*"], p, full_grammar=True, subset=np.array([3, 4]))
    name, c = ix.fake.calls[-1]
    assert name == "np_hip_search_hybrid_expr" and c["n_sub"] == 1 and len(c["queries"][0]["nodes"]) == 5
    # the entries without an _expr form say so
    with pytest.raises(ValueError, match="no _expr form yet"):
        ix.search_hybrid_grouped(qs, [tree, "ab"], p)


def test_cpp_mirror_reaches_the_same_entries(tmp_path):
    """tests/cpp/text_expr_binding_check.cpp: next_plaid.hpp against recording stubs, with the host compiler alone and under
    ASan + UBSan (an array the header sized too small is an error there)."""
    exe = tmp_path / "text_expr_binding_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "text_expr_binding_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
