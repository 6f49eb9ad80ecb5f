"""The host side of the keyword half of a hybrid search (text_search.rs): reading an FTS5 index into the arrays
np_hip_index_set_text takes, the crate's query sanitizers and identifier tokenizer, and the compiler from FTS5 query text to
the term-id phrases np_hip_text_search takes.  Pure host code: sqlite3 and numpy, no device, no library.

The keyword index is SQLite's own: fts5vocab(..., 'instance') lists every (term, document, position) of an FTS5 table, tokenised
by SQLite itself, so the device scores exactly the tokens SQLite would.  Query text is tokenised the same way, through a
scratch FTS5 table with the index's tokenize= clause."""
from __future__ import annotations

import sqlite3
from dataclasses import dataclass, field

import numpy as np

FTS_TABLE = "METADATA_FTS"
FTS_CONTENT_TABLE = "METADATA_FTS_CONTENT"
FTS_CONTENT_COLUMN = "_fts_content_"
FTS_CONFIG_TABLE = "_FTS_SETTINGS_"

NP_TEXT_AND, NP_TEXT_OR = 0, 1
NP_TEXT_MAX_PHRASES, NP_TEXT_MAX_TOKENS, NP_TEXT_MAX_TOPK = 64, 256, 1024
NP_FUSE_RRF, NP_FUSE_RELATIVE_SCORE = 0, 1
FUSION_MODES = {"rrf": NP_FUSE_RRF, "relative_score": NP_FUSE_RELATIVE_SCORE}

# FtsTokenizer (text_search.rs:60-104): the name in the settings table -> the FTS5 tokenize= value
TOKENIZERS = {"unicode61": "unicode61", "trigram": "trigram", "identifier_aware": "unicode61"}


class TextQueryError(ValueError):
    """An FTS5 query that compile_text_query does not translate (it never approximates one); the message names the construct."""


# ---- the identifier-aware tokenizer (text_search.rs:118-258) -------------------------------------------------------------

def _camel_split(token: str) -> list[str]:
    """camelCase / PascalCase parts, lowercase: digit runs, an acronym before a capitalised word (HTTPResponse -> http,
    response), capitalised or lowercase words.  ASCII only, as the reference works on bytes."""
    parts, i, n = [], 0, len(token)
    is_up = lambda ch: "A" <= ch <= "Z"
    is_lo = lambda ch: "a" <= ch <= "z"
    while i < n:
        c = token[i]
        if "0" <= c <= "9":
            j = i
            while i < n and "0" <= token[i] <= "9":
                i += 1
            parts.append(token[j:i])
        elif is_up(c):
            j = i
            while i + 1 < n and is_up(token[i + 1]):
                i += 1
            if i + 1 < n and is_lo(token[i + 1]) and i > j:   # the last capital opens the next word
                parts.append(token[j:i].lower())
                continue
            i += 1
            while i < n and is_lo(token[i]):
                i += 1
            parts.append(token[j:i].lower())
        elif is_lo(c):
            j = i
            while i < n and is_lo(token[i]):
                i += 1
            parts.append(token[j:i])
        else:
            i += 1
    return parts


def split_identifier(token: str) -> list[str]:
    """The lowered compound, then -- if it has at least two parts -- every part and the adjacent pairs joined by '_':
    HandlerStack -> handlerstack, handler, stack, handler_stack."""
    lower = token.lower()
    parts = [p for p in lower.split("_") if p] if "_" in token else _camel_split(token)
    if len(parts) < 2:
        return [lower]
    return [lower] + parts + [f"{a}_{b}" for a, b in zip(parts, parts[1:])]


def tokenize_identifiers(text: str) -> list[str]:
    """tokenize_identifiers (text_search.rs:218-246): identifiers are [A-Za-z_][A-Za-z0-9_]*, ASCII only (the reference
    scans bytes; no byte of a multi-byte UTF-8 character is an ASCII letter), everything else separates; each identifier is
    expanded by split_identifier."""
    out, i, n = [], 0, len(text)
    head = lambda ch: ("a" <= ch <= "z") or ("A" <= ch <= "Z") or ch == "_"
    while i < n:
        if head(text[i]):
            j = i
            i += 1
            while i < n and (head(text[i]) or "0" <= text[i] <= "9"):
                i += 1
            out.extend(split_identifier(text[j:i]))
        else:
            i += 1
    return out


def prepare_document_text(text: str, tokenizer: str) -> str:
    """What the crate hands FTS5 for a document body (text_search.rs:252-257)."""
    return " ".join(tokenize_identifiers(text)) if tokenizer == "identifier_aware" else text


# ---- the query sanitizers (text_search.rs:949-993) -----------------------------------------------------------------------

def sanitize_fts5_query(query: str) -> str:
    """sanitize_fts5_query: whitespace-separated words, edges trimmed of non-alphanumeric characters, the FTS5 operators
    dropped, each word double-quoted; implicit AND.  Edge trimming follows Rust's char::is_alphanumeric for ASCII and
    Latin-1 (where str.isalnum agrees with it) and is unchecked beyond: the two may disagree on a few other code points."""
    out = []
    for word in query.split():
        a, b = 0, len(word)
        while a < b and not word[a].isalnum():
            a += 1
        while b > a and not word[b - 1].isalnum():
            b -= 1
        w = word[a:b]
        if not w or w.upper() in ("AND", "OR", "NOT", "NEAR"):
            continue
        out.append('"' + w.replace('"', '""') + '"')
    return " ".join(out)


def sanitize_fts5_query_or(query: str) -> str:
    """sanitize_fts5_query_or: the identifier tokens of the query, each once in order of first appearance, double-quoted
    and joined by OR (for an identifier_aware index)."""
    seen, out = set(), []
    for tok in tokenize_identifiers(query):
        if tok and tok not in seen:
            seen.add(tok)
            out.append('"' + tok.replace('"', '""') + '"')
    return " OR ".join(out)


# ---- unicode61 beyond ASCII: SQLite's own rule as a table ------------------------------------------------------------------
# unicode61 (remove_diacritics=1, the default) is context-free per code point but for one thing: a combining mark continues
# a token that is open and separates otherwise.  So three classes and one folded code point per code point describe it, and
# probing the SQLite that from_texts itself uses gives them: the document 'x' + chr(cp) + 'y' comes back as the tokens
# ['x', 'y'] (cp separates), ['x?y'] (a token character; ? is its fold, always one code point) or ['xy'] (a mark: it
# continued the token and left nothing in the term).  Nothing of SQLite's source tables is written down here.
UNICODE_PLANE = 65536
UNICODE_SEPARATOR, UNICODE_TOKEN, UNICODE_MARK = 0, 1, 2
UNICODE_FOLD_MASK = 0x1FFFFF
# plane -> its 65536 entries, and planes -> the table of that many planes: filled once per process.  Two threads that ask
# first at the same time may both probe a plane; the results are equal and the last one stored stays, which is harmless.
_UNICODE61_PLANES: dict = {}
_UNICODE61_TABLES: dict = {}
unicode61_probe_seconds: dict = {}    # plane -> what its probe took (tools/textbuild_time.py --utf8 reports it)


def _probe_unicode61_plane(plane: int) -> np.ndarray:
    import time
    t0 = time.perf_counter()
    out = np.zeros(UNICODE_PLANE, np.uint32)
    first = plane * UNICODE_PLANE
    cps = [cp for cp in range(first, first + UNICODE_PLANE) if cp != 0 and not 0xD800 <= cp < 0xE000]
    conn = sqlite3.connect(":memory:")
    try:
        conn.execute("CREATE VIRTUAL TABLE s USING fts5(c, tokenize='unicode61')")
        conn.execute("CREATE VIRTUAL TABLE sv USING fts5vocab('s', 'instance')")
        conn.executemany("INSERT INTO s(rowid, c) VALUES (?, ?)", ((cp, "x" + chr(cp) + "y") for cp in cps))
        toks: dict = {}
        for term, doc, _ in conn.execute("SELECT term, doc, offset FROM sv ORDER BY doc, offset"):
            toks.setdefault(doc, []).append(term)
    finally:
        conn.close()
    for cp in cps:
        got = toks.get(cp, [])
        if got == ["x", "y"]:
            continue                                   # class 0, fold 0
        if got == ["xy"]:
            out[cp - first] = UNICODE_MARK << 30
        elif len(got) == 1 and len(got[0]) == 3 and got[0][0] == "x" and got[0][2] == "y":
            out[cp - first] = (UNICODE_TOKEN << 30) | ord(got[0][1])
        else:
            raise ValueError(f"unicode61_table: SQLite {sqlite3.sqlite_version} tokenises 'x' + U+{cp:04X} + 'y' as {got!r}, "
                             f"which the three classes do not describe")
    unicode61_probe_seconds[plane] = time.perf_counter() - t0
    return out


def unicode61_table(planes: int = 2) -> np.ndarray:
    """SQLite's unicode61 rule for the code points of the first `planes` planes (1..17), as np_text_build_opts.unicode_table
    takes it: uint32 [planes * 65536], bits 0-20 the folded code point, bits 30-31 the class -- 0 a separator (the whole
    entry is 0; code point 0 and the surrogates among them), 1 a token character, 2 a mark (it continues an open token,
    contributes nothing to the term and separates otherwise).  Probed from the SQLite of this process one plane at a time
    (a fraction of a second each) and cached per process; the result is read-only."""
    planes = int(planes)
    if not 1 <= planes <= 17:
        raise ValueError(f"unicode61_table: planes {planes} outside 1..17")
    got = _UNICODE61_TABLES.get(planes)
    if got is None:
        for p in range(planes):
            if p not in _UNICODE61_PLANES:
                _UNICODE61_PLANES[p] = _probe_unicode61_plane(p)
        got = np.concatenate([_UNICODE61_PLANES[p] for p in range(planes)])
        got.setflags(write=False)
        _UNICODE61_TABLES[planes] = got
    return got


# ---- the keyword index as arrays -----------------------------------------------------------------------------------------

@dataclass
class TextIndexData:
    """An FTS5 index as np_hip_index_set_text takes it, plus the vocabulary (which stays on the host).  Term ids number the
    terms in fts5vocab's order."""
    tokenizer: str                    # the crate's name: unicode61, trigram, identifier_aware
    terms: list                       # term id -> term
    term_offsets: np.ndarray          # int64 [n_terms + 1]
    inst_doc: np.ndarray              # int64 [instances] rowids
    inst_pos: np.ndarray              # int32 [instances]
    n_rows: int                       # FTS5's nRow
    vocab: dict = field(default_factory=dict)
    build_report: dict = field(default=None, repr=False, compare=False)    # from_texts_device: the stage report ...
    fallback_docs: list = field(default=None, repr=False, compare=False)   # ... and the documents SQLite tokenised
    _scratch: object = field(default=None, repr=False, compare=False)
    _cache: dict = field(default_factory=dict, repr=False, compare=False)

    resident = False                  # ResidentTextIndexData: the arrays lie in a handle's HBM

    @property
    def tokenize(self) -> str:
        return TOKENIZERS[self.tokenizer]

    @property
    def n_terms(self) -> int:
        return len(self.terms)

    @classmethod
    def _read(cls, conn, table: str, tokenizer: str, schema: str = "main") -> "TextIndexData":
        conn.execute(f"CREATE VIRTUAL TABLE temp._np_vocab USING fts5vocab('{schema}', '{table}', 'instance')")
        try:
            rows = conn.execute("SELECT term, doc, offset FROM temp._np_vocab").fetchall()
        finally:
            conn.execute("DROP TABLE temp._np_vocab")
        n_rows = int(conn.execute(f'SELECT count(*) FROM "{table}_docsize"').fetchone()[0])
        terms, starts = [], []
        for i, r in enumerate(rows):
            if not terms or r[0] != terms[-1]:
                terms.append(r[0])
                starts.append(i)
        vocab = {t: i for i, t in enumerate(terms)}
        if len(vocab) != len(terms):
            raise ValueError("fts5vocab did not list every term's instances together")
        off = np.asarray(starts + [len(rows)], np.int64)
        doc = np.asarray([r[1] for r in rows], np.int64).reshape(-1)
        pos = np.asarray([r[2] for r in rows], np.int32).reshape(-1)
        return cls(tokenizer, terms, off, doc, pos, n_rows, vocab)

    @classmethod
    def from_sqlite(cls, db_path: str) -> "TextIndexData":
        """The METADATA_FTS table of a metadata.db the crate wrote (text_search.rs:306-500): its instances, the tokenizer
        named in _FTS_SETTINGS_ (unicode61 where the table has no such row) and its row count.  The file is opened read-only."""
        conn = sqlite3.connect(f"file:{db_path}?mode=ro", uri=True)
        try:
            if conn.execute("SELECT count(*) FROM sqlite_master WHERE name = ?", (FTS_TABLE,)).fetchone()[0] == 0:
                raise ValueError(f"{db_path} has no {FTS_TABLE} table")
            tok = "unicode61"
            if conn.execute("SELECT count(*) FROM sqlite_master WHERE name = ?", (FTS_CONFIG_TABLE,)).fetchone()[0]:
                row = conn.execute(f'SELECT value FROM "{FTS_CONFIG_TABLE}" WHERE key = \'tokenizer\'').fetchone()
                if row is not None:
                    tok = row[0]
            if tok not in TOKENIZERS:
                raise ValueError(f"{db_path}: unknown tokenizer {tok!r} in {FTS_CONFIG_TABLE}")
            return cls._read(conn, FTS_TABLE, tok)
        finally:
            conn.close()

    @classmethod
    def from_texts(cls, texts, tokenizer: str = "unicode61", content_synced: bool = False) -> "TextIndexData":
        """An in-memory FTS5 table over `texts` (document i = rowid i), read the same way.  identifier_aware passes every
        text through tokenize_identifiers first, as the crate does.  content_synced builds the crate's layout (an
        external-content table) instead of a plain FTS5 table; the index is the same."""
        if tokenizer not in TOKENIZERS:
            raise ValueError(f"unknown tokenizer {tokenizer!r}")
        conn = sqlite3.connect(":memory:")
        try:
            create_fts_tables(conn, tokenizer, content_synced=content_synced)
            insert_fts_rows(conn, list(texts), range(len(texts)), tokenizer, content_synced=content_synced)
            return cls._read(conn, FTS_TABLE, tokenizer)
        finally:
            conn.close()

    @classmethod
    def from_texts_device(cls, texts, tokenizer: str = "unicode61", device: int = 0, max_token_bytes: int | None = None,
                          utf8: bool = False, unicode_planes: int = 2, **knobs) -> "TextIndexData":
        """from_texts without the FTS5 table: the documents are tokenised, their terms numbered and the instances sorted on
        the device (np_hip_text_build), and the arrays equal from_texts' one for one.  The device reproduces SQLite for
        ASCII text (trigram: without NUL; unicode61: tokens of at most max_token_bytes, 256 unless given); the documents it
        hands back -- fallback_docs on the result -- go through a scratch FTS5 table here and are merged in.
        identifier_aware expands identifiers on the host first, as from_texts does.  build_report holds the stage report.
        utf8=True hands the library unicode61_table(unicode_planes): unicode61 and identifier_aware are then reproduced for
        all well-formed UTF-8 inside those planes (max_token_bytes counts raw bytes, at most 21845), and only documents with
        a code point beyond them or an overlong token fall back; trigram is as without it.
        `knobs` are the test knobs of np_text_build_opts (hash_bits, tile_bytes, workspace_bytes)."""
        if tokenizer not in TOKENIZERS:
            raise ValueError(f"unknown tokenizer {tokenizer!r}")
        from . import api   # the one module that calls the library; resolved here so that this one imports without it
        texts = list(texts)
        raws = [prepare_document_text(t, tokenizer).encode("utf-8") for t in texts]
        off = np.zeros(len(raws) + 1, np.int64)
        if raws:
            off[1:] = np.cumsum([len(r) for r in raws])
        raw = np.frombuffer(b"".join(raws), np.uint8)

        def tokenize_fallback(ids):
            return _tokenize_rows(cls, [texts[int(i)] for i in ids], [int(i) for i in ids], tokenizer)

        code = api.NP_TOK_TRIGRAM if TOKENIZERS[tokenizer] == "trigram" else api.NP_TOK_UNICODE61
        r = api.text_build(raw, off, code, tokenize_fallback, device=device, max_token_bytes=int(max_token_bytes or 0),
                           utf8=utf8, unicode_planes=unicode_planes, **knobs)
        return cls._of_build(tokenizer, r)

    @classmethod
    def _of_build(cls, tokenizer: str, r: dict) -> "TextIndexData":
        tb, tbo = r["term_bytes"].tobytes(), r["term_byte_offsets"]
        terms = [tb[tbo[i]: tbo[i + 1]].decode("utf-8") for i in range(tbo.size - 1)]
        data = cls(tokenizer, terms, r["term_offsets"], r["inst_doc"], r["inst_pos"], r["n_rows"],
                   {t: i for i, t in enumerate(terms)})
        data.build_report = r["report"]
        data.fallback_docs = [int(i) for i in r["fallback_docs"]]
        return data

    def updated(self, new_texts=(), *, delete=(), replace=None, renumber: bool = True, n_rows: int | None = None,
                device: int = 0, max_token_bytes: int | None = None, utf8: bool = False, unicode_planes: int = 2,
                **knobs) -> "TextIndexData":
        """The index of the table after the crate's index / delete / update_rows (and rebuild), without building it again:
        a new TextIndexData, equal array for array to from_texts of the resulting rows.  `delete` lists row ids that go,
        `replace` maps row ids to their new text ({id: text} or (id, text) pairs), `new_texts` are appended behind the last
        id.  The batch -- the replacements in id order, then new_texts -- is built on the device as from_texts_device does
        (fallback documents through SQLite) and merged into this index there (np_hip_text_build_merge).
        renumber=True numbers the surviving rows 0, 1, ... in order, as `delete` + `rebuild` leave them (and as the document
        ids of the vector index are after a delete); renumber=False keeps every id, holes included.
        The table must be dense -- rows 0 .. self.n_rows - 1, which is what from_texts and a renumbered update leave --
        unless n_rows names the size of its id space (the ids then in use are the caller's knowledge: every id in `delete`
        and `replace` must be a row, and renumber=True is refused).  build_report is the merge's report (under "batch": the
        report of the batch's build, None without a batch), fallback_docs index the batch.  utf8 / unicode_planes: as
        from_texts_device takes them, for the batch.  `knobs`: from_texts_device's, and merge_workspace_bytes."""
        from . import api
        remap, delta_ids, n_rows_out, raw, off, code, tokenize_fallback = self._update_plan(new_texts, delete, replace, renumber, n_rows)
        tokenizer, cls = self.tokenizer, type(self)
        r = api.text_merge([t.encode("utf-8") for t in self.terms], self.term_offsets, self.inst_doc, self.inst_pos, int(self.n_rows),
                           remap, delta_ids, n_rows_out, raw, off, code, tokenize_fallback,
                           device=device, max_token_bytes=int(max_token_bytes or 0), utf8=utf8, unicode_planes=unicode_planes,
                           **knobs)
        data = cls._of_build(tokenizer, r)
        data.build_report = dict(r["report"], batch=r["build_report"])     # the merge's report; the batch's build inside it
        return data

    def _update_plan(self, new_texts, delete, replace, renumber, n_rows):
        """updated()'s arguments checked and turned into what the merge entries take: (remap, delta_ids, n_rows_out, the
        batch's bytes and offsets or None, the tokenizer code, tokenize_fallback).  A resident index's arrays are not read."""
        from . import api
        tokenizer = self.tokenizer
        n_old = int(self.n_rows) if n_rows is None else int(n_rows)
        if n_old < int(self.n_rows):
            raise ValueError(f"updated: n_rows {n_old} is below the table's {int(self.n_rows)} rows")
        if n_rows is not None and renumber and n_old != int(self.n_rows):
            raise ValueError("updated: renumber=True needs a dense table (rows 0 .. n_rows - 1); pass renumber=False")
        if not self.resident and self.inst_doc.size and int(self.inst_doc.max()) >= n_old:
            raise ValueError(f"updated: the index names document {int(self.inst_doc.max())} but the table has {n_old} row ids; "
                             f"a table with holes needs n_rows")
        gone = sorted(set(int(d) for d in delete))
        rep = sorted((int(k), v) for k, v in (replace.items() if isinstance(replace, dict) else (replace or ())))
        rep_ids = [k for k, _ in rep]
        if len(set(rep_ids)) != len(rep_ids):
            raise ValueError("updated: an id is replaced twice")
        for d in gone + rep_ids:
            if d < 0 or d >= n_old:
                raise ValueError(f"updated: row {d} is outside the table's {n_old} row ids")
        both = set(gone) & set(rep_ids)
        if both:
            raise ValueError(f"updated: row {min(both)} is in both delete and replace")
        new_texts = list(new_texts)
        texts = [t for _, t in rep] + new_texts
        # the survivors' new ids; a replaced row keeps its place in the order but leaves the base
        remap = np.arange(n_old, dtype=np.int64)
        remap[gone] = -1
        if renumber:
            alive = remap >= 0
            remap[alive] = np.arange(int(alive.sum()), dtype=np.int64)
            top = int(alive.sum())
        else:
            top = n_old
        delta_ids = np.concatenate([remap[rep_ids], top + np.arange(len(new_texts), dtype=np.int64)]).astype(np.int64)
        remap[rep_ids] = -1
        n_rows_out = int(self.n_rows) - len(gone) + len(new_texts)
        raws = [prepare_document_text(t, tokenizer).encode("utf-8") for t in texts]
        off = np.zeros(len(raws) + 1, np.int64)
        if raws:
            off[1:] = np.cumsum([len(r) for r in raws])
        raw = np.frombuffer(b"".join(raws), np.uint8)
        cls = TextIndexData if self.resident else type(self)

        def tokenize_fallback(ids):
            return _tokenize_rows(cls, [texts[int(i)] for i in ids], [int(i) for i in ids], tokenizer)

        code = api.NP_TOK_TRIGRAM if TOKENIZERS[tokenizer] == "trigram" else api.NP_TOK_UNICODE61
        return remap, delta_ids, n_rows_out, raw if texts else None, off if texts else None, code, tokenize_fallback

    # -- tokenising query text with the index's tokenizer -------------------------------------------------
    def tokens_of(self, phrase: str) -> list[str]:
        """The tokens SQLite's tokenizer makes of a string, in position order (through a scratch FTS5 table)."""
        got = self._cache.get(phrase)
        if got is not None:
            return got
        if self._scratch is None:
            self._scratch = sqlite3.connect(":memory:", check_same_thread=False)
            self._scratch.execute(f"CREATE VIRTUAL TABLE s USING fts5(c, tokenize='{self.tokenize}')")
            self._scratch.execute("CREATE VIRTUAL TABLE sv USING fts5vocab('s', 'instance')")
        c = self._scratch
        c.execute("DELETE FROM s")
        c.execute("INSERT INTO s(rowid, c) VALUES (1, ?)", (phrase,))
        got = [r[0] for r in c.execute("SELECT term FROM sv ORDER BY offset").fetchall()]
        if len(self._cache) < 65536:
            self._cache[phrase] = got
        return got

    def term_ids(self, phrase: str) -> list[int]:
        return [self.vocab.get(t, -1) for t in self.tokens_of(phrase)]


class ResidentTextIndexData(TextIndexData):
    """The keyword index of a handle that was built or updated in HBM (MmapIndex.build_text / update_text with
    resident=True): terms, vocab, n_rows and tokenizer as on any TextIndexData, so that compile_text_query,
    compile_text_expr, prefix_range and set_text_shard work on it; term_offsets, inst_doc and inst_pos are fetched from the
    handle on first access (np_hip_index_get_text) and then kept.  A later resident update of the handle gives it a new
    object and INVALIDATES the arrays of the one it replaces unless they were fetched before: reading them then raises."""
    resident = True

    def __init__(self, tokenizer, terms, n_rows, fetch, build_report=None, fallback_docs=None):
        self.tokenizer, self.terms, self.n_rows = tokenizer, terms, int(n_rows)
        self.vocab = {t: i for i, t in enumerate(terms)}
        self.build_report, self.fallback_docs = build_report, fallback_docs
        self._scratch, self._cache = None, {}
        self._fetch, self._arrays = fetch, None

    def _get(self, i):
        if self._arrays is None:
            if self._fetch is None:
                raise ValueError("this keyword index was replaced by a later resident update before its arrays were fetched: "
                                 "read MmapIndex.text (or get_text()) instead")
            self._arrays = self._fetch()
            self._fetch = None
        return self._arrays[i]

    def invalidate(self):
        """The handle holds another keyword index now: arrays that were not fetched cannot be any more."""
        self._fetch = None

    term_offsets = property(lambda self: self._get(0))
    inst_doc = property(lambda self: self._get(1))
    inst_pos = property(lambda self: self._get(2))

    def __repr__(self):
        return f"ResidentTextIndexData(tokenizer={self.tokenizer!r}, n_terms={len(self.terms)}, n_rows={self.n_rows})"

    def __eq__(self, other):
        return self is other

    __hash__ = object.__hash__


def _tokenize_rows(cls, texts, ids, tokenizer: str):
    """The instances SQLite makes of `texts` at rowids `ids`, as np_hip_text_build_add takes the fallback documents':
    (term_bytes u8, term_byte_offsets i64, inst_term i32, inst_doc i64, inst_pos i32), through a scratch FTS5 table."""
    conn = sqlite3.connect(":memory:")
    try:
        create_fts_tables(conn, tokenizer, content_synced=False)
        insert_fts_rows(conn, texts, ids, tokenizer, content_synced=False)
        d = cls._read(conn, FTS_TABLE, tokenizer)
    finally:
        conn.close()
    enc = [t.encode("utf-8") for t in d.terms]
    tbo = np.zeros(len(enc) + 1, np.int64)
    if enc:
        tbo[1:] = np.cumsum([len(t) for t in enc])
    inst_term = np.repeat(np.arange(len(enc), dtype=np.int32), np.diff(d.term_offsets))
    return np.frombuffer(b"".join(enc), np.uint8), tbo, inst_term, d.inst_doc, d.inst_pos


def create_fts_tables(conn, tokenizer: str, content_synced: bool = True):
    """The tables of text_search.rs:306-384 (ensure_tables) in plain SQL: the settings table, the content table and the
    FTS5 table over it -- or, content_synced=False, a plain FTS5 table of the same name and column."""
    conn.execute(f'CREATE TABLE IF NOT EXISTS "{FTS_CONFIG_TABLE}" (key TEXT PRIMARY KEY, value TEXT NOT NULL)')
    if content_synced:
        conn.execute(f'CREATE TABLE IF NOT EXISTS "{FTS_CONTENT_TABLE}" (rowid INTEGER PRIMARY KEY, '
                     f'"{FTS_CONTENT_COLUMN}" TEXT NOT NULL DEFAULT \'\')')
        conn.execute(f'CREATE VIRTUAL TABLE IF NOT EXISTS "{FTS_TABLE}" USING fts5("{FTS_CONTENT_COLUMN}", '
                     f"content='{FTS_CONTENT_TABLE}', content_rowid='rowid', tokenize='{TOKENIZERS[tokenizer]}')")
    else:
        conn.execute(f'CREATE VIRTUAL TABLE IF NOT EXISTS "{FTS_TABLE}" USING fts5("{FTS_CONTENT_COLUMN}", '
                     f"tokenize='{TOKENIZERS[tokenizer]}')")
    conn.execute(f'INSERT OR REPLACE INTO "{FTS_CONFIG_TABLE}"(key, value) VALUES (\'tokenizer\', ?)', (tokenizer,))


def insert_fts_rows(conn, texts, doc_ids, tokenizer: str, content_synced: bool = True):
    """insert_rows (text_search.rs:386-440): the raw text into the content table, the prepared text into the FTS5 table."""
    with conn:
        for doc_id, text in zip(doc_ids, texts):
            if content_synced:
                conn.execute(f'INSERT OR REPLACE INTO "{FTS_CONTENT_TABLE}"(rowid, "{FTS_CONTENT_COLUMN}") VALUES (?, ?)',
                             (int(doc_id), text))
            conn.execute(f'INSERT INTO "{FTS_TABLE}"(rowid, "{FTS_CONTENT_COLUMN}") VALUES (?, ?)',
                         (int(doc_id), prepare_document_text(text, tokenizer)))


# ---- FTS5 query text -> phrases of term ids --------------------------------------------------------------------------------

@dataclass
class TextQuery:
    """A compiled keyword query (np_text_query): phrase p owns terms[phrase_offsets[p] : phrase_offsets[p + 1]], -1 = a token
    the vocabulary does not hold; mode NP_TEXT_AND or NP_TEXT_OR."""
    terms: np.ndarray            # int32
    phrase_offsets: np.ndarray   # int32 [n_phrases + 1]
    mode: int = NP_TEXT_AND

    @property
    def n_phrases(self) -> int:
        return int(self.phrase_offsets.size) - 1

    @classmethod
    def from_phrases(cls, phrases, mode: int = NP_TEXT_AND) -> "TextQuery":
        phrases = [list(p) for p in phrases]
        off = np.zeros(len(phrases) + 1, np.int32)
        if phrases:
            off[1:] = np.cumsum([len(p) for p in phrases])
        flat = [t for p in phrases for t in p]
        return cls(np.asarray(flat, np.int32).reshape(-1), off, int(mode))

    def phrases(self) -> list:
        return [self.terms[self.phrase_offsets[i]: self.phrase_offsets[i + 1]].tolist() for i in range(self.n_phrases)]


MATCH_NOTHING = [[-1]]   # one phrase of one unknown token: the compiled form of a query that matches no document


def _bareword_char(ch: str) -> bool:
    return ch.isascii() and (ch.isalnum() or ch == "_") or ord(ch) >= 0x80 or ch == "\x1a"


def _lex(text: str):
    """(kind, value) items: ('phrase', string) for a double-quoted string or a bareword, ('op', 'AND' | 'OR')."""
    items, i, n = [], 0, len(text)
    special = {"(": "parentheses", ")": "parentheses", "*": "a prefix query (*)", "^": "an initial-token query (^)",
               ":": "a column filter (:)", "{": "a column filter ({})", "}": "a column filter ({})", "-": "a column filter (-)",
               "+": "phrase concatenation (+)", ",": "a NEAR argument list (,)"}
    while i < n:
        ch = text[i]
        if ch in " \t\n\r":
            i += 1
        elif ch == '"':
            j, buf = i + 1, []
            while True:
                if j >= n:
                    raise TextQueryError("an unterminated string")
                if text[j] == '"':
                    if j + 1 < n and text[j + 1] == '"':
                        buf.append('"')
                        j += 2
                        continue
                    break
                buf.append(text[j])
                j += 1
            items.append(("phrase", "".join(buf)))
            i = j + 1
        elif _bareword_char(ch):
            j = i
            while j < n and _bareword_char(text[j]):
                j += 1
            word = text[i:j]
            k = j
            while k < n and text[k] in " \t\n\r":
                k += 1
            if word == "NOT":
                raise TextQueryError("NOT")
            if word == "NEAR" and k < n and text[k] == "(":
                raise TextQueryError("NEAR")
            items.append(("op", word) if word in ("AND", "OR") else ("phrase", word))
            i = j
        elif ch in special:
            raise TextQueryError(special[ch])
        else:
            raise TextQueryError(f"the character {ch!r} outside a string (an FTS5 syntax error)")
    return items


def parse_text_query(text: str):
    """The shape of a query compile_text_query accepts: (groups, mode) where mode is NP_TEXT_AND or NP_TEXT_OR and groups is
    a list of lists of phrase strings -- for AND, the runs of adjacent phrases between explicit ANDs; for OR, one phrase per
    group.  Raises TextQueryError for anything else."""
    items = _lex(text)
    if not items:
        raise TextQueryError("an empty query (an FTS5 syntax error)")
    groups, ops, want_phrase = [[]], set(), True
    for kind, val in items:
        if kind == "op":
            if want_phrase:
                raise TextQueryError(f"{val} without a phrase before it (an FTS5 syntax error)")
            ops.add(val)
            groups.append([])
            want_phrase = True
        else:
            groups[-1].append(val)
            want_phrase = False
    if want_phrase:
        raise TextQueryError("an operator without a phrase after it (an FTS5 syntax error)")
    if len(ops) > 1:
        raise TextQueryError("AND mixed with OR")
    if ops == {"OR"} and any(len(g) > 1 for g in groups):
        raise TextQueryError("OR mixed with implicit AND")
    return groups, (NP_TEXT_OR if ops == {"OR"} else NP_TEXT_AND)


def compile_text_query(text: str, data: TextIndexData) -> TextQuery:
    """FTS5 query text -> TextQuery, for what the two sanitizers emit and what people type: double-quoted phrases or bare
    words, joined all by AND (implicit, explicit or both) or all by OR.  Each phrase is tokenised by SQLite's own tokenizer
    with the index's tokenize= clause, so a word the tokenizer splits (parse_request under unicode61, any word under
    trigram) becomes a phrase of several tokens.  NOT, NEAR, *, ^, column filters, parentheses, + and AND mixed with OR
    raise TextQueryError naming the construct; nothing is approximated.

    A phrase without tokens ("" or "!!!", or fewer than three characters under trigram) does what SQLite 3.37 does with it:
    among phrases joined by OR or by implicit AND it is dropped; a side of an explicit AND that holds nothing else makes the
    whole query match nothing, and so does a query all of whose phrases are empty.  A query that matches nothing compiles
    to one phrase of one unknown token."""
    groups, mode = parse_text_query(text)
    phrases, nothing = [], False
    for g in groups:
        kept = [ids for ids in (data.term_ids(p) for p in g) if ids]
        if not kept and mode == NP_TEXT_AND:
            nothing = True
        phrases += kept
    if nothing or not phrases:
        return TextQuery.from_phrases(MATCH_NOTHING, NP_TEXT_AND)
    if len(phrases) > NP_TEXT_MAX_PHRASES:
        raise TextQueryError(f"more than {NP_TEXT_MAX_PHRASES} phrases")
    if sum(len(p) for p in phrases) > NP_TEXT_MAX_TOKENS:
        raise TextQueryError(f"more than {NP_TEXT_MAX_TOKENS} tokens")
    return TextQuery.from_phrases(phrases, mode)


# ---- FTS5 query text -> a tree of phrases (the boolean grammar and prefix queries) -------------------------------------------

NP_TEXT_NODE_PHRASE, NP_TEXT_NODE_AND, NP_TEXT_NODE_OR, NP_TEXT_NODE_NOT = 0, 1, 2, 3
NP_TEXT_MAX_NODES = 127
NP_TEXT_MAX_PREFIX_TERMS = 1024   # terms a prefix may stand for at the end of a phrase of several tokens
_NODE_OPS = {"and": NP_TEXT_NODE_AND, "or": NP_TEXT_NODE_OR, "not": NP_TEXT_NODE_NOT}


@dataclass
class TextExpr:
    """A compiled keyword query with FTS5's boolean operators (np_text_expr): the phrases as TextQuery has them, in the
    order of the query text; prefix[p] = None, or the range (lo, hi) of term ids the phrase's last token stands for (the
    token itself is then lo, or -1 where the range is empty: such a phrase never occurs); nodes = the tree in postfix order,
    rows of (op, a, b): NP_TEXT_NODE_PHRASE names phrase a, AND / OR / NOT name their left and right child rows.  NOT is
    binary: a AND NOT b.  The last row is the root."""
    terms: np.ndarray            # int32
    phrase_offsets: np.ndarray   # int32 [n_phrases + 1]
    prefix: list                 # [n_phrases] None | (lo, hi)
    nodes: np.ndarray            # int32 [n_nodes, 3]

    @property
    def n_phrases(self) -> int:
        return int(self.phrase_offsets.size) - 1

    @property
    def n_nodes(self) -> int:
        return int(self.nodes.shape[0])

    def phrases(self) -> list:
        return [self.terms[self.phrase_offsets[i]: self.phrase_offsets[i + 1]].tolist() for i in range(self.n_phrases)]

    def prefix_hi(self) -> np.ndarray:
        """np_text_expr.prefix_hi: the end of a phrase's range, 0 for an exact last token (and for an empty range, whose
        last token is -1)."""
        return np.asarray([0 if r is None or r[1] <= r[0] else r[1] for r in self.prefix], np.int32).reshape(-1)

    @classmethod
    def from_tree(cls, tree) -> "TextExpr":
        """tree = ("phrase", term ids[, (lo, hi)]) or (op, left, right) with op "and", "or" or "not".  The last token of a
        prefix phrase is overwritten with the start of its range."""
        phrases, prefix, nodes = [], [], []

        def walk(t):
            if t[0] == "phrase":
                ids, rng = list(t[1]), (tuple(t[2]) if len(t) > 2 and t[2] is not None else None)
                if rng is not None:
                    ids[-1] = int(rng[0]) if rng[1] > rng[0] else -1
                phrases.append(ids)
                prefix.append(rng)
                nodes.append((NP_TEXT_NODE_PHRASE, len(phrases) - 1, 0))
            else:
                a = walk(t[1])
                b = walk(t[2])
                nodes.append((_NODE_OPS[t[0]], a, b))
            return len(nodes) - 1

        walk(tree)
        off = np.zeros(len(phrases) + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in phrases])
        flat = [x for p in phrases for x in p]
        return cls(np.asarray(flat, np.int32).reshape(-1), off, prefix, np.asarray(nodes, np.int32).reshape(-1, 3))

    @classmethod
    def from_query(cls, query: TextQuery) -> "TextExpr":
        """A flat TextQuery as a tree: its phrases chained from the left by AND or by OR."""
        tree = None
        for p in query.phrases():
            leaf = ("phrase", p)
            tree = leaf if tree is None else ("and" if query.mode == NP_TEXT_AND else "or", tree, leaf)
        return cls.from_tree(tree)


def _lex_expr(text: str):
    """Tokens of the full grammar: ('str', value) for a double-quoted string or a bareword, ('AND' | 'OR' | 'NOT' | '(' | ')' |
    '*' | '+', None).  NEAR, ^ and column filters raise TextQueryError by name."""
    items, i, n = [], 0, len(text)
    refused = {"^": "an initial-token query (^)", ":": "a column filter (:)", "{": "a column filter ({})",
               "}": "a column filter ({})", "-": "a column filter (-)", ",": "a NEAR argument list (,)"}
    while i < n:
        ch = text[i]
        if ch in " \t\n\r":
            i += 1
        elif ch == '"':
            j, buf = i + 1, []
            while True:
                if j >= n:
                    raise TextQueryError("an unterminated string")
                if text[j] == '"':
                    if j + 1 < n and text[j + 1] == '"':
                        buf.append('"')
                        j += 2
                        continue
                    break
                buf.append(text[j])
                j += 1
            items.append(("str", "".join(buf)))
            i = j + 1
        elif _bareword_char(ch):
            j = i
            while j < n and _bareword_char(text[j]):
                j += 1
            word = text[i:j]
            k = j
            while k < n and text[k] in " \t\n\r":
                k += 1
            if word == "NEAR" and k < n and text[k] == "(":
                raise TextQueryError("NEAR")
            items.append((word, None) if word in ("AND", "OR", "NOT") else ("str", word))
            i = j
        elif ch in "()*+":
            items.append((ch, None))
            i += 1
        elif ch in refused:
            raise TextQueryError(refused[ch])
        else:
            raise TextQueryError(f"the character {ch!r} outside a string (an FTS5 syntax error)")
    return items


def parse_text_expr(text: str):
    """The tree of an FTS5 query with SQLite's precedence: implicit AND (between phrases only) binds tightest, then NOT,
    then AND, then OR, all from the left.  Returns nested tuples: ("phrase", [strings joined by +], prefix flag),
    ("list", [phrases]) for a run of phrases joined by implicit AND, (op, left, right)."""
    items = _lex_expr(text)
    if not items:
        raise TextQueryError("an empty query (an FTS5 syntax error)")
    pos = 0

    def peek():
        return items[pos][0] if pos < len(items) else None

    def phrase():
        nonlocal pos
        parts, star = [items[pos][1]], False
        pos += 1
        while True:
            if peek() == "*":
                if star:
                    raise TextQueryError("* after * (an FTS5 syntax error)")
                star = True
                pos += 1
            elif peek() == "+":
                if star:
                    raise TextQueryError("a prefix (*) before the end of a phrase")
                pos += 1
                if peek() != "str":
                    raise TextQueryError("+ without a string after it (an FTS5 syntax error)")
                parts.append(items[pos][1])
                pos += 1
            else:
                break
        if peek() == "(":
            raise TextQueryError("a phrase followed by ( (an FTS5 syntax error)")
        return ("phrase", parts, star)

    def primary():
        nonlocal pos
        if peek() == "(":
            pos += 1
            e = expr(0)
            if peek() != ")":
                raise TextQueryError("an unbalanced ( (an FTS5 syntax error)")
            pos += 1
            if peek() in ("str", "("):
                raise TextQueryError("an expression in parentheses followed by a phrase or ( (an FTS5 syntax error: implicit "
                                     "AND joins phrases only)")
            return e
        if peek() != "str":
            raise TextQueryError(f"{peek() or 'the end of the query'} where a phrase is expected (an FTS5 syntax error)")
        run = [phrase()]
        while peek() == "str":
            run.append(phrase())
        return ("list", run)

    level = {"OR": 1, "AND": 2, "NOT": 3}

    def expr(min_level):
        nonlocal pos
        left = primary()
        while peek() in level and level[peek()] >= min_level:
            op = peek()
            pos += 1
            right = expr(level[op] + 1)
            left = (op.lower(), left, right)
        return left

    tree = expr(0)
    if pos != len(items):
        raise TextQueryError(f"{items[pos][0]} where the query should end (an FTS5 syntax error)")
    return tree


def _term_bytes(data: TextIndexData):
    """The vocabulary as UTF-8 bytes, checked once to ascend (fts5vocab lists terms in byte order): what makes the terms
    that start with a prefix one range of term ids."""
    enc = data._cache.get(("term bytes",))
    if enc is None:
        enc = [t.encode("utf-8") for t in data.terms]
        if any(a >= b for a, b in zip(enc, enc[1:])):
            raise ValueError("the vocabulary is not in ascending byte order: a prefix is no range of term ids")
        data._cache[("term bytes",)] = enc
    return enc


def prefix_range(token: str, data: TextIndexData):
    """(lo, hi): the term ids whose terms start with `token`; lo == hi where none does."""
    import bisect
    enc, pre = _term_bytes(data), token.encode("utf-8")
    lo = bisect.bisect_left(enc, pre)
    end = pre.rstrip(b"\xff")
    hi = len(enc) if not end else bisect.bisect_left(enc, end[:-1] + bytes([end[-1] + 1]))
    return lo, max(lo, hi)


def compile_text_expr(text: str, data: TextIndexData) -> TextExpr:
    """FTS5 query text -> TextExpr: phrases (double-quoted or bare words, joined by + into one phrase), * after a phrase
    (its last token becomes a prefix), implicit AND between phrases, NOT, AND, OR and parentheses, with SQLite's precedence.
    Each phrase is tokenised by the index's own tokenizer.  NEAR, ^, column filters and FTS5 syntax errors raise
    TextQueryError naming the construct, and so do a prefix under the trigram tokenizer, a * before the end of a phrase,
    more than 64 phrases, more than 256 tokens, and a phrase of several tokens whose prefix stands for more than
    NP_TEXT_MAX_PREFIX_TERMS terms.

    A phrase without tokens does what SQLite 3.37 does with it: in a run of phrases joined by implicit AND it is dropped;
    a run that holds nothing else, like an operand of AND, OR or NOT that is such a phrase, matches no document (it compiles
    to a phrase of one unknown token)."""
    tree = parse_text_expr(text)
    count = {"phrases": 0, "tokens": 0}

    def leaf(ids, rng=None):
        count["phrases"] += 1
        count["tokens"] += len(ids)
        return ("phrase", ids, rng)

    def build(t):
        if t[0] == "list":
            kept = []
            for _, parts, star in t[1]:
                if star and data.tokenize == "trigram":
                    raise TextQueryError("a prefix query (*) under the trigram tokenizer")
                ids, toks = [], []
                for s in parts:
                    toks += data.tokens_of(s)
                ids = [data.vocab.get(x, -1) for x in toks]
                if not ids:
                    continue
                rng = None
                if star:
                    rng = prefix_range(toks[-1], data)
                    if len(ids) > 1 and rng[1] - rng[0] > NP_TEXT_MAX_PREFIX_TERMS:
                        raise TextQueryError(f"a phrase of several tokens ending in a prefix of {rng[1] - rng[0]} terms (more "
                                             f"than NP_TEXT_MAX_PREFIX_TERMS = {NP_TEXT_MAX_PREFIX_TERMS})")
                kept.append(leaf(ids, rng))
            if not kept:
                return leaf([-1])
            out = kept[0]
            for k in kept[1:]:
                out = ("and", out, k)
            return out
        return (t[0], build(t[1]), build(t[2]))

    built = build(tree)
    if count["phrases"] > NP_TEXT_MAX_PHRASES:
        raise TextQueryError(f"more than {NP_TEXT_MAX_PHRASES} phrases")
    if count["tokens"] > NP_TEXT_MAX_TOKENS:
        raise TextQueryError(f"more than {NP_TEXT_MAX_TOKENS} tokens")
    return TextExpr.from_tree(built)
