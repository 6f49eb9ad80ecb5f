"""Metadata filters at their limits: more than 256 entries in the table of (filter, document chunk) totals and more than 256
compaction blocks in one chunk (the carry between the tiles of filter_block_scan), programs of stack depth 32 and of 256 ops
(filter_mask_kernel's two stack registers) and IN lists of 5 000 constants (filter_in's binary search).  Needs a real MI355X.

The reference is tests/filter_restate.py (pinned to SQLite by tests/test_filter_restate_cpu.py) or, at 4.2 M documents,
numpy directly; ids equal."""
import numpy as np
import pytest

from helpers import hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import api, filters as F, text as T
import filter_restate as R

pytestmark = pytest.mark.gpu

BLOCK_DOCS = 16384   # documents per compaction block (NP_FILTER_BLOCK_DOCS)
TILE = 256           # entries filter_block_scan takes at a time (FILTER_TPB)
STAGED_UNIT = BLOCK_DOCS // 8 + 4 + 8 + 8 * BLOCK_DOCS   # bytes per (filter, block) of np_hip_filter_eval (filter_block_bytes)


def tiny(n_docs, **opts):
    """An index of n_docs one-token documents: the filters only need its document count."""
    spec, a = make_arrays(num_docs=n_docs, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    return spec, a, hip_index(a, **opts)


def one_word_text(n):
    """Every document is the one word w: a keyword search returns the lowest ids of its scope."""
    return T.TextIndexData("unicode61", ["w"], np.array([0, n], np.int64), np.arange(n, dtype=np.int64), np.zeros(n, np.int32), n, {"w": 0})


# ---- 1: more than 256 entries in the table ---------------------------------------------------------------------------------

def conditions_300():
    conds = R.random_conditions(296, seed=33)
    for at, c in ((0, "1=1"), (255, "0=1"), (256, "1=1"), (299, "0=1")):    # around the tile boundary and at both ends
        conds.insert(at, (c, []))
    assert len(conds) == 300 and conds[0][0] == "1=1" and conds[255][0] == "0=1" and conds[256][0] == "1=1" and conds[299][0] == "0=1"
    return conds


@pytest.fixture(scope="module")
def rows_70001():
    return R.make_rows(70001)


@pytest.mark.parametrize("n,opts", [(4099, {}), (70001, {"workspace_bytes": 300_000})], ids=["4099", "70001-chunks"])
def test_300_filters_in_one_call(n, opts, rows_70001):
    """4 099 documents are one chunk of documents: 300 entries.  70 001 with 300 kB run one staged (filter, block) unit at a
    time: 300 chunks of filters times 5 chunks of documents, 1 500 entries."""
    rows = rows_70001 if n == 70001 else R.make_rows(n)
    spec, a, hx = tiny(n, **opts)
    try:
        hx.set_columns(rows)
        sch = hx.schema
        conds = conditions_300()
        progs = [npa.compile_filter(c, p, sch) for c, p in conds]
        assert len(progs) > TILE                                            # (times the chunks of documents, whatever they are)
        want = [R.select(p, sch) for p in progs]
        got = hx.filter_ids(progs)
        assert len(got) == 300
        for j, ((c, p), g, w) in enumerate(zip(conds, got, want)):
            assert g.dtype == np.int64 and np.array_equal(g, w), f"n={n} filter {j} {c} {p}: {g[:8]} ({g.size}) vs {w[:8]} ({w.size})"
        assert got[0].size == n and got[255].size == 0 and got[256].size == n and got[299].size == 0
        assert sum(0 < w.size < n for w in want) > 100
        assert np.array_equal(hx.filter_ids(progs, counts_only=True), [w.size for w in want])
        if not opts:
            # the same conditions as the filters of a search, one query per filter: the CSR that stays on the device
            distinct, qf = api.pack_filters(progs, 300, sch)
            assert len(distinct) > TILE
            hx.set_text(one_word_text(n))
            q = T.TextQuery.from_phrases([[0]])
            res = hx.text_search([q] * 300, 10, filters=progs)
            for j, (r, w) in enumerate(zip(res, want)):
                assert np.array_equal(r.passage_ids, w[:10]), f"text_search, filter {j} {conds[j]}: {r.passage_ids} vs {w[:10]}"
            qs, _ = synth.make_queries(spec, 1, n_tokens=4, cen=a["centroids"])
            ex = hx.search_exact([qs[0]] * 300, 5, filters=progs)
            by = hx.search_exact([qs[0]] * 300, 5, subsets=want)
            for j, (r, s) in enumerate(zip(ex, by)):
                assert r.passage_ids.tobytes() == s.passage_ids.tobytes() and r.scores.tobytes() == s.scores.tobytes(), f"search_exact, filter {j}"
                assert np.isin(r.passage_ids, want[j]).all() and r.passage_ids.size == min(5, want[j].size)
    finally:
        hx.close()


# ---- 2: more than 256 compaction blocks in one chunk -----------------------------------------------------------------------

def test_more_than_256_blocks_in_one_chunk():
    n = 258 * BLOCK_DOCS + 5
    edge = TILE * BLOCK_DOCS                                                # the first document of the scan's second tile
    spec, a, hx = tiny(n)
    try:
        docno = np.arange(n, dtype=np.int64)
        x = (docno % 11).astype(np.float64)
        x[::7] = np.nan
        hx.set_columns({"docno": docno, "z": docno % 5, "x": x})
        conds = [("1=1", []), ("z = ?", [4]), ("docno >= ?", [n - 1]), ("x IS NULL", []), ("docno BETWEEN ? AND ?", [edge - 3, edge + 3])]
        want = [docno, docno[docno % 5 == 4], docno[-1:], docno[::7], np.arange(edge - 3, edge + 4)]
        # one chunk: the default workspace holds 5 filters x 259 blocks of the id-staging pass beside the programs and tables
        blocks = -(-n // BLOCK_DOCS)
        assert blocks == 259 and blocks > TILE
        assert (hx.workspace_bytes() - (1 << 20)) // STAGED_UNIT // len(conds) >= blocks
        got = hx.filter_ids(conds)
        for (c, p), g, w in zip(conds, got, want):
            assert g.dtype == np.int64 and g.size == w.size and np.array_equal(g, w), f"{c} {p}: {g[:8]} ({g.size}) vs {w[:8]} ({w.size})"
        assert np.array_equal(hx.filter_ids(conds, counts_only=True), [w.size for w in want])
        qs, _ = synth.make_queries(spec, 1, n_tokens=4, cen=a["centroids"])
        f = hx.search_exact([qs[0]], 10, filters=[conds[4]])[0]
        s = hx.search_exact([qs[0]], 10, subsets=[want[4]])[0]
        assert f.passage_ids.tobytes() == s.passage_ids.tobytes() and f.scores.tobytes() == s.scores.tobytes()
        assert sorted(f.passage_ids.tolist()) == want[4].tolist()
    finally:
        hx.close()


# ---- 3: the deepest and the longest programs -------------------------------------------------------------------------------

def leaf(kind, col=-1, arg=0, vals=()):
    return kind, col, arg, list(vals)


def program(items):
    """items: leaves as leaf() gives them and the ops NP_F_AND / NP_F_OR / NP_F_NOT as integers -> CompiledFilter."""
    ops, values = [], []
    for it in items:
        if isinstance(it, tuple):
            kind, col, arg, vals = it
            ops.append((kind, col, arg, len(vals), len(values) if vals else 0))
            values += vals
        else:
            ops.append((it, -1, 0, 0, 0))
    return F.CompiledFilter(ops, np.asarray(values, np.int64).reshape(-1))


def depth_of(prog):
    d = top = 0
    for op, *_ in prog.ops:
        d += -1 if op in (F.NP_F_AND, F.NP_F_OR) else 0 if op == F.NP_F_NOT else 1
        top = max(top, d)
    assert d == 1
    return top


def bits_of(v):
    return int(np.float64(v).view(np.int64))


def deep_items(cols, negate, swap, last=None):
    """32 leaves, then 31 operators: the first combines leaves 30 and 31 at the top of the stack, the last leaf 0 with all
    the rest.  Operators alternate AND / OR from the top; leaves under an AND are mostly TRUE, under an OR mostly FALSE, with
    NULL outcomes among both (y and w have validity arrays), so that the value at the bottom depends on the two at the top."""
    y, z, w = cols["y"], cols["z"], cols["w"]
    true_ish = [leaf(F.NP_F_CMP, z, 5, [0]), leaf(F.NP_F_CONST, arg=F.CONST_TRUE), leaf(F.NP_F_CMP, y, 4, [R.I64_MIN]),   # y > min: NULL rows unknown
                leaf(F.NP_F_BETWEEN, z, 0, [0, 4]), leaf(F.NP_F_CMP, w, 2, [bits_of(50.0)])]
    false_ish = [leaf(F.NP_F_CMP, z, 2, [0]), leaf(F.NP_F_CONST, arg=F.CONST_FALSE), leaf(F.NP_F_IS_NULL, y),
                 leaf(F.NP_F_CMP, w, 4, [bits_of(2.5)]), leaf(F.NP_F_IN, y, 0, [7, 19])]
    leaves = [(true_ish[(k // 2) % len(true_ish)] if k % 2 == 0 else false_ish[(k // 2) % len(false_ish)]) for k in range(30)]
    leaves += last or [leaf(F.NP_F_CMP, y, 4, [0]), leaf(F.NP_F_CMP, w, 4, [bits_of(0.0)])]    # y > 0, w > 0: TRUE, FALSE and NULL rows
    items = []
    for l in leaves:
        items.append(l)
        if negate:
            items.append(F.NP_F_NOT)
    a, o = (F.NP_F_OR, F.NP_F_AND) if swap else (F.NP_F_AND, F.NP_F_OR)
    items += [a if j % 2 == 0 else o for j in range(31)]
    return items


@pytest.fixture(scope="module", params=[65, 4099])
def columns(request):
    n = request.param
    rows = R.make_rows(n, seed=n)
    rng = np.random.default_rng(n)
    d = np.arange(n, dtype=np.int64)
    cols = {"y": rows["y"], "z": rows["z"], "w": rows["w"], "d": np.ma.MaskedArray(d, rng.random(n) < 0.2),
            "u": np.ma.MaskedArray(d * 0.5, rng.random(n) < 0.2)}
    spec, a, hx = tiny(n)
    hx.set_columns(cols)
    yield n, hx, hx.schema, {name: c.index for name, c in hx.schema.columns.items()}
    hx.close()


def test_stack_depth_32(columns):
    n, hx, sch, ci = columns
    assert sch["y"].valid is not None and sch["w"].valid is not None and sch["y"].type == F.NP_COL_I64 and sch["w"].type == F.NP_COL_F64
    plain = deep_items(ci, False, False)
    negated = deep_items(ci, True, False)
    mirrored = deep_items(ci, True, True)                                   # NOT on every leaf, AND and OR exchanged: NOT of the whole
    fixed = [deep_items(ci, False, False, [leaf(F.NP_F_CONST, arg=x), leaf(F.NP_F_CONST, arg=y)])
             for x, y in ((F.CONST_TRUE, F.CONST_TRUE), (F.CONST_FALSE, F.CONST_TRUE), (F.CONST_TRUE, F.CONST_UNKNOWN))]
    # every program also with a NOT at its end: what it selects then tells a FALSE at the bottom from a NULL
    progs = [program(items + tail) for items in [plain, negated, mirrored] + fixed for tail in ([], [F.NP_F_NOT])]
    assert all(depth_of(p) == F.MAX_DEPTH == 32 for p in progs) and len(progs[0].ops) == 63 and len(progs[2].ops) == 95
    want = [R.select(p, sch) for p in progs]
    t, k = R.evaluate(progs[0], sch)
    # the result at the bottom follows the two entries at the top of the stack: TRUE, FALSE and NULL all occur, and fixing
    # those entries to (TRUE, TRUE), (FALSE, TRUE) or (TRUE, NULL) gives three other results
    assert (t & k).any() and (~t & k).any() and (~k).any()
    assert np.array_equal(want[1], np.nonzero(~t & k)[0]) and np.array_equal(want[4], want[1]) and np.array_equal(want[5], want[0])
    assert len({want[j].tobytes() + b"|" + want[j + 1].tobytes() for j in (0, 6, 8, 10)}) == 4
    got = hx.filter_ids(progs)
    for j, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"n={n} program {j}: {g[:8]} ({g.size}) vs {w[:8]} ({w.size})"


def test_256_ops_and_in_lists_of_5000(columns):
    n, hx, sch, ci = columns
    y, z, w, d, u = (ci[c] for c in "yzwdu")
    # 128 leaves joined left to right, AND and OR alternating, and a NOT: 1 + 127 * 2 + 1 = 256 ops
    pool = [leaf(F.NP_F_CMP, y, 4, [-3]), leaf(F.NP_F_CMP, z, 1, [2]), leaf(F.NP_F_CMP, w, 2, [bits_of(0.25)]), leaf(F.NP_F_IS_NULL, d),
            leaf(F.NP_F_BETWEEN, d, 0, [n // 3, n // 2]), leaf(F.NP_F_IN, y, 1, [1, 7]), leaf(F.NP_F_CMP, u, 5, [bits_of(n / 8)])]
    items = [pool[0]]
    for i in range(1, 128):
        items += [pool[(i * 3) % len(pool)], F.NP_F_AND if i % 2 else F.NP_F_OR]
    longest = program(items + [F.NP_F_NOT])
    assert len(longest.ops) == F.MAX_OPS == 256
    # IN lists of 5 000 ascending constants: every third document number, with and without a NULL in the list, plain and negated
    ints = [3 * i for i in range(5000)]
    halves = [bits_of(1.5 * i) for i in range(5000)]
    ins = []
    for col, vals in ((d, ints), (u, halves)):
        for flag in (0, 1):
            ins += [program([leaf(F.NP_F_IN, col, flag, vals)]), program([leaf(F.NP_F_IN, col, flag, vals), F.NP_F_NOT])]
    progs = [longest] + ins
    want = [R.select(p, sch) for p in progs]
    for col, base in (("d", 1), ("u", 5)):
        valid = sch[col].valid.astype(bool)
        third = np.arange(n) % 3 == 0
        assert np.array_equal(want[base], np.nonzero(valid & third)[0]) and np.array_equal(want[base + 2], want[base])
        assert np.array_equal(want[base + 1], np.nonzero(valid & ~third)[0]) and want[base + 3].size == 0   # NOT IN (.., NULL) selects nothing
    assert 0 < want[0].size < n
    got = hx.filter_ids(progs)
    for j, (g, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g, w_), f"n={n} program {j}: {g[:8]} ({g.size}) vs {w_[:8]} ({w_.size})"
