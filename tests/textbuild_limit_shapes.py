"""The corpora of tests/test_gpu_textbuild_limits.py -- the device keyword-index build and merge at the constants of their own
kernels -- and the vectorised reference for the shapes SQLite is too slow for.  tests/test_textbuild_limits_cpu.py runs the
same generators at a reduced size and pins the reference to SQLite, to tests/textbuild_restate.py and to
tests/textmerge_restate.py, array for array.  Every generator takes its size as a parameter.

A word corpus is (words, flat, row_off): `words` the sorted list of distinct byte strings ([0-9a-z] only), `flat` the word index
of every token of every row in order, `row_off` [n_rows + 1] where each row's tokens lie in `flat`.  Its text joins a row's
words with one space.

The reference (ref_build, ref_update) states the index directly: the instances are the (row id, position) pairs, a position is
the token's ordinal in its row, and the index is their stable sort by word; a word without an instance is no term."""
import sqlite3

import numpy as np

from next_plaid_amd import text as T
from next_plaid_amd.text import TextIndexData

SCAN_CHUNK = 2048      # NP_TB_SCAN_CHUNK: items per block of a scan launch
SCAN_ROUND = 256       # block sums that tb_scan_sums takes per round
SORT_CHUNK = 2048      # NP_TB_SORT_CHUNK: keys per block of a radix pass
MAX_PROBES = 1024      # TB_MAX_PROBES
MAX_TOKEN = 32768      # NP_TEXT_BUILD_MAX_TOKEN_BYTES, and FTS5's own token limit

REF_DEFECTS = ("unstable_sort", "byte_pos", "ids_not_renumbered", "dead_term_kept")


def blocks(n, per=SCAN_CHUNK):
    return -(-int(n) // per)


# ---- comparing two indexes ---------------------------------------------------------------------------------------------------
def assert_same(got, want):
    assert got.terms == want.terms, ([t for t in got.terms if t not in want.vocab][:5], [t for t in want.terms if t not in got.vocab][:5])
    assert np.array_equal(got.term_offsets, want.term_offsets)
    assert np.array_equal(got.inst_doc, want.inst_doc)
    assert np.array_equal(got.inst_pos, want.inst_pos)
    assert got.n_rows == want.n_rows and got.vocab == want.vocab
    assert got.term_offsets.dtype == np.int64 and got.inst_doc.dtype == np.int64 and got.inst_pos.dtype == np.int32


def rows_after(texts, new_texts=(), delete=(), replace=None, renumber=True):
    """{row id: text} of the table after the update, stated independently of the binding."""
    gone = set(delete)
    rows = {i: t for i, t in enumerate(texts) if i not in gone}
    rows.update(replace or {})
    if renumber:
        rows = {n: rows[d] for n, d in enumerate(sorted(rows))}
        top = len(rows)
    else:
        top = len(texts)
    rows.update({top + i: t for i, t in enumerate(new_texts)})
    return rows


def sqlite_rows(rows, tokenizer="unicode61"):
    conn = sqlite3.connect(":memory:")
    try:
        T.create_fts_tables(conn, tokenizer, content_synced=False)
        ids = sorted(rows)
        T.insert_fts_rows(conn, [rows[i] for i in ids], ids, tokenizer, content_synced=False)
        return TextIndexData._read(conn, T.FTS_TABLE, tokenizer)
    finally:
        conn.close()


def flat_index(d):
    """An index as values that compare bit for bit."""
    return (tuple(d.terms), d.term_offsets.tobytes(), d.inst_doc.tobytes(), d.inst_pos.tobytes(), int(d.n_rows),
            tuple(d.fallback_docs or ()))


# ---- word corpora: bytes, texts and the reference ----------------------------------------------------------------------------
def csr(rows):
    """[[word index, ...], ...] -> (flat, row_off)."""
    row_off = np.zeros(len(rows) + 1, np.int64)
    row_off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.asarray([w for r in rows for w in r], np.int64).reshape(-1)
    return flat, row_off


def token_bytes(words, flat, row_off):
    """Per token, the bytes it takes in the row's text: the word, and the space behind it unless it ends the row."""
    size = np.asarray([len(w) for w in words], np.int64)[flat] + 1
    ends = row_off[1:][row_off[1:] > row_off[:-1]] - 1
    size[ends] -= 1
    return size


def raw_of(words, flat, row_off):
    """(the rows' texts concatenated as u8, byte offsets [n_rows + 1]) without a Python string per row."""
    flat, row_off = np.asarray(flat, np.int64), np.asarray(row_off, np.int64)
    width = max(len(w) for w in words) + 1
    table = np.full((len(words), width), 0x20, np.uint8)
    for i, w in enumerate(words):
        table[i, : len(w)] = np.frombuffer(w, np.uint8)
    size = token_bytes(words, flat, row_off)
    raw = table[flat][np.arange(width)[None, :] < size[:, None]]
    at = np.concatenate([[0], np.cumsum(size)])
    return np.ascontiguousarray(raw), at[row_off].astype(np.int64)


def texts_of(raw, off):
    b = raw.tobytes()
    return [b[off[i]: off[i + 1]].decode("ascii") for i in range(off.size - 1)]


def as_data(a, tokenizer="unicode61"):
    """arrays (byte-string terms) -> a TextIndexData."""
    terms = [t.decode("ascii") for t in a["terms"]]
    return TextIndexData(tokenizer, terms, a["term_offsets"], a["inst_doc"], a["inst_pos"], int(a["n_rows"]),
                         {t: i for i, t in enumerate(terms)})


def _index_of(words, word, ids, pos, order, n_rows, keep_dead):
    count = np.bincount(word, minlength=len(words)).astype(np.int64)
    alive = np.ones(len(words), bool) if keep_dead else count > 0
    off = np.concatenate([[0], np.cumsum(count[alive])]).astype(np.int64)
    return dict(terms=[w for w, a in zip(words, alive) if a], term_offsets=off, inst_doc=ids[order].astype(np.int64),
                inst_pos=pos[order].astype(np.int32), n_rows=int(n_rows))


def _positions(words, flat, row_off, defect):
    doc = np.repeat(np.arange(row_off.size - 1, dtype=np.int64), np.diff(row_off))
    if defect == "byte_pos":
        size = token_bytes(words, flat, row_off)
        start = np.concatenate([[0], np.cumsum(size)])
        return doc, (start[:-1] - start[row_off[doc]]).astype(np.int64)
    return doc, np.arange(flat.size, dtype=np.int64) - row_off[doc]


def ref_build(words, flat, row_off, defect=None):
    """The index of the word corpus: row i is document i."""
    flat, row_off = np.asarray(flat, np.int64), np.asarray(row_off, np.int64)
    doc, pos = _positions(words, flat, row_off, defect)
    if defect == "unstable_sort":       # by word alone, from an input that is not in (document, position) order
        order = (flat.size - 1 - np.argsort(flat[::-1], kind="stable")).astype(np.int64)
    else:
        order = np.argsort(flat, kind="stable")
    return _index_of(words, flat, doc, pos, order, row_off.size - 1, defect == "dead_term_kept")


def ref_update(words, flat, row_off, batch_flat, batch_off, n_replace, delete=(), replace_ids=(), renumber=True, defect=None):
    """The index of the table after TextIndexData.updated: the rows in `delete` go, the rows in `replace_ids` (ascending) get the
    first n_replace rows of the batch, the rest of the batch is appended behind the last id.  Stated on the table, not on the
    two indexes: the rows that stay keep their tokens and get their new id, then everything is ordered by (word, id, position)."""
    flat, row_off = np.asarray(flat, np.int64), np.asarray(row_off, np.int64)
    batch_flat, batch_off = np.asarray(batch_flat, np.int64), np.asarray(batch_off, np.int64)
    n_old, n_batch = row_off.size - 1, batch_off.size - 1
    replace_ids = np.asarray(sorted(replace_ids), np.int64)
    assert replace_ids.size == n_replace <= n_batch
    there = np.ones(n_old, bool)
    there[np.asarray(list(delete), np.int64)] = False
    new_id = np.arange(n_old, dtype=np.int64)
    if renumber and defect != "ids_not_renumbered":
        new_id = np.cumsum(there) - 1
    top = int(there.sum()) if renumber else n_old
    batch_ids = np.concatenate([new_id[replace_ids], top + np.arange(n_batch - n_replace, dtype=np.int64)])
    stays = there.copy()
    stays[replace_ids] = False
    doc_a, pos_a = _positions(words, flat, row_off, defect)
    doc_b, pos_b = _positions(words, batch_flat, batch_off, defect)
    sel = stays[doc_a]
    word = np.concatenate([flat[sel], batch_flat])
    ids = np.concatenate([new_id[doc_a[sel]], batch_ids[doc_b]])
    pos = np.concatenate([pos_a[sel], pos_b])
    order = np.lexsort((pos, ids, word))
    return _index_of(words, word, ids, pos, order, int(there.sum()) + n_batch - n_replace, defect == "dead_term_kept")


# ---- B1: scans above one round -----------------------------------------------------------------------------------------------
def sparse_corpus(n_docs, edge):
    """n_docs documents, all empty except every 97th ("a b{i % 5}"), the documents edge - 1, edge, edge + 1 and the last: the
    scan of the per-document counts has live entries on both sides of `edge` and in a ragged last round."""
    texts = [""] * n_docs
    for i in list(range(0, n_docs, 97)) + [edge - 1, edge, edge + 1, n_docs - 1]:
        texts[i] = f"a b{i % 5}"
    return texts


def wide_table_corpus(n_docs=300, seed=12):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(500)]
    return [" ".join(rng.choice(words, int(rng.integers(0, 30)))) for _ in range(n_docs)]


# ---- B2: the histogram scan above one round ----------------------------------------------------------------------------------
def one_long_document(n_tokens, seed=2, n_words=300):
    """One document of n_tokens tokens drawn from n_words two-letter words, and a short second document."""
    rng = np.random.default_rng(seed)
    letters = "abcdefghijklmnopqrstuvwxyz"
    words = sorted((letters[i // 26] + letters[i % 26]).encode() for i in range(n_words))
    first = rng.integers(0, n_words, n_tokens)
    k = min(n_words, n_tokens)
    first[:k] = rng.permutation(n_words)[:k]      # every word occurs (n_tokens >= n_words)
    flat = np.concatenate([first, [3, 0, 3]]).astype(np.int64)
    return words, flat, np.asarray([0, n_tokens, n_tokens + 3], np.int64)


# ---- B3: a table that is full at TB_MAX_PROBES -------------------------------------------------------------------------------
def many_terms_corpus(n_terms, n_docs=200, seed=3):
    """n_terms distinct terms, each twice, shuffled over n_docs documents."""
    rng = np.random.default_rng(seed)
    toks = rng.permutation(np.repeat(np.arange(n_terms), 2))
    cut = np.linspace(0, toks.size, n_docs + 1).astype(int)
    return [" ".join(f"t{int(v)}" for v in toks[cut[d]: cut[d + 1]]) for d in range(n_docs)]


# ---- B4: full-wave tiles and the token cap -----------------------------------------------------------------------------------
TILE_LEADS = (0, 1, 7, 8, 15, 16)


def tile_edge_corpus(tile, leads=TILE_LEADS):
    """tests/test_gpu_textbuild.py::test_tokens_at_and_across_tile_edges scaled to `tile`: tokens that begin or end at tile - 1,
    tile and tile + 1 (and at the second edge) or straddle it; after each lead a document of `lead` bytes shifts every later
    document against the 16-byte lines the walk loads."""
    texts = []
    for lead in leads:
        for edge in (tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1):
            for tok in (1, 2, 3, tile, tile + 5, 3 * tile + 1):
                for start in (edge - tok, edge - tok + 1, edge - 1, edge):
                    if start < 0:
                        continue
                    texts.append("-" * start + "T" * tok + " z")
        texts.append("q" * lead)
    return texts


def token_cap_corpus(cap):
    """Tokens of exactly `cap` bytes ("x") and of cap + 1 ("y"), alone and inside text, at leads 0 and 7.  Returns the texts and
    the documents that hold a token over the cap."""
    texts, over = [], []
    for lead in (0, 7):
        for n, c in ((cap, "x"), (cap + 1, "y")):
            for text in ("-" * lead + c * n, "-" * lead + "a " + c * n + " b"):
                if n > cap:
                    over.append(len(texts))
                texts.append(text)
        texts.append("ok")
    return texts, over


# ---- B5: trigram, three passes -----------------------------------------------------------------------------------------------
def random_bytes_document(n_bytes, seed=1):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(1, 0x80, n_bytes).astype(np.uint8)).decode("ascii"), "abc"]


# ---- B6: the planned workspace -----------------------------------------------------------------------------------------------
def workspace_corpus(n_docs=100, per_doc=200, seed=6):
    rng = np.random.default_rng(seed)
    words = [f"k{i}" for i in range(700)]
    return [" ".join(rng.choice(words, per_doc)) for _ in range(n_docs)]


# ---- M1: the merge's S above one round ---------------------------------------------------------------------------------------
RUN_WORDS = sorted(w.encode() for w in ("a", "first", "last", "m", "mid", "new", "other", "q", "x", "zz"))
_W = {w: i for i, w in enumerate(RUN_WORDS)}


def _ids(text):
    return [_W[w.encode()] for w in text.split()]


def run_corpus(edge, tail, lead):
    """test_gpu_textmerge.py::_run_corpus with the chunk edge at instance `edge`: "m" once in each of edge + tail documents, up
    to document edge - 2, which holds it four times.  `lead` instances of "a" in document 3 shift the run."""
    n = edge + tail
    m, lens = _W[b"m"], np.ones(n, np.int64)
    big = edge - 2
    special = {big: _ids("m m x m m"), 3: _ids("a " * lead + "m"), 7: _ids("m zz")}
    for d, r in special.items():
        lens[d] = len(r)
    row_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.full(int(row_off[-1]), m, np.int64)
    for d, r in special.items():
        flat[row_off[d]: row_off[d + 1]] = r
    return RUN_WORDS, flat, row_off, big


def run_update(base, edge, n, big):
    """The update of M1 on the base index `base` (arrays): the documents whose "m" instance sits at instance edge - 1, edge and
    edge + 1, the first, the last and the neighbours of the four-instance document go; one document below, one between and one
    above the edge is replaced; two rows are appended."""
    at = np.asarray([edge - 1, edge, edge + 1])
    t = base["terms"].index(b"m")
    assert base["term_offsets"][t] <= at[0] and at[-1] < base["term_offsets"][t + 1]
    delete = sorted(set(int(d) for d in base["inst_doc"][at]) | {0, n - 1, big - 1, big + 1})
    replace = {min(1000, big // 2): "m other m", big + 5: "mid m", n - 2: "last"}
    replace = {k: v for k, v in replace.items() if k not in delete}
    new = ["m new", "q m m"]
    batch = [_ids(replace[k]) for k in sorted(replace)] + [_ids(t_) for t_ in new]
    return delete, replace, new, csr(batch)


# ---- P1: the corpora of the threads ------------------------------------------------------------------------------------------
def thread_corpus(n_docs=300, seed=21):
    rng = np.random.default_rng(seed)
    words = [f"wo{i}" for i in range(12)] + ["Alpha", "beta9", "x"]
    return [" ".join(rng.choice(words, int(rng.integers(0, 14)))) for _ in range(n_docs)]
