"""unicode61 beyond ASCII restated from text.unicode61_table alone: three classes per code point (separator, token
character with a one-code-point fold, mark) and one rule of context -- a mark continues a token that is open and separates
otherwise.  This is what the device's UTF-8 walk implements; the tests hold it against SQLite itself, and each planted
DEFECT (a way the kernels could get it wrong) must change an answer.

Also here: SQLite's tokens of many short documents in one scratch table, the random strings of the CPU and GPU tests, and
the prediction of the fallback list (malformed UTF-8, a code point beyond the table, a token of too many raw bytes)."""
import random
import sqlite3


from next_plaid_amd import text as T

DEFECTS = ("mark_starts_token", "mark_after_separator_continues", "fold_not_applied", "continuation_byte_on_its_own",
           "cap_on_folded_bytes")


class Model:
    def __init__(self, planes: int = 2):
        t = T.unicode61_table(planes)
        self.table = t
        self.cls = (t >> 30).tolist()
        self.fold = (t & T.UNICODE_FOLD_MASK).tolist()

    def tokens(self, text: str, defect: str | None = None):
        """[(term, first raw byte, raw bytes)] in position order.  Every code point of `text` lies inside the table."""
        out, term, start, at, open_ = [], [], 0, 0, False
        for ch in text:
            cp, n = ord(ch), len(ch.encode("utf-8"))
            c = self.cls[cp]
            if defect == "continuation_byte_on_its_own" and n > 1 and c != T.UNICODE_SEPARATOR:
                # the lead byte took the code point's class; every byte behind it is looked up as a code point of its own
                if any(self.cls[b] != T.UNICODE_TOKEN for b in ch.encode("utf-8")[1:]):
                    c = T.UNICODE_SEPARATOR
            if c == T.UNICODE_TOKEN:
                if not open_:
                    term, start, open_ = [], at, True
                term.append(ch if defect == "fold_not_applied" else chr(self.fold[cp]))
            elif c == T.UNICODE_MARK and open_:
                pass                                   # continues the token, adds nothing to the term
            elif c == T.UNICODE_MARK and ((defect == "mark_starts_token" and at == 0) or
                                          (defect == "mark_after_separator_continues" and at > 0)):
                term, start, open_ = [], at, True      # (a token of marks alone shows as an empty term)
            else:
                if open_:
                    out.append(("".join(term), start, at - start))
                open_ = False
            at += n
        if open_:
            out.append(("".join(term), start, at - start))
        return out

    def terms(self, text: str, defect: str | None = None):
        return [t for t, _, _ in self.tokens(text, defect)]

    def overlong(self, text: str, max_token_bytes: int, defect: str | None = None) -> bool:
        """The cap's verdict: a token of more than max_token_bytes RAW bytes sends the document to the fallback list."""
        if defect == "cap_on_folded_bytes":
            return any(len(t.encode("utf-8")) > max_token_bytes for t, _, _ in self.tokens(text))
        return any(n > max_token_bytes for _, _, n in self.tokens(text))


def well_formed(raw: bytes) -> bool:
    """Strict UTF-8: no stray continuation, overlong form, surrogate, value above U+10FFFF, F8..FF or cut sequence."""
    try:
        raw.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def predict_fallback(raws, planes: int = 2, max_token_bytes: int = 256, model: Model | None = None):
    """The ids of the documents (raw bytes each) the device hands back in UTF-8 mode."""
    model = model or Model(planes)
    out = []
    for i, raw in enumerate(raws):
        if not well_formed(raw):
            out.append(i)
            continue
        s = raw.decode("utf-8")
        if any(ord(ch) >= planes * T.UNICODE_PLANE for ch in s) or model.overlong(s, max_token_bytes):
            out.append(i)
    return out


def sqlite_terms(texts):
    """SQLite's unicode61 tokens of every text, in position order: one scratch FTS5 table for all of them."""
    conn = sqlite3.connect(":memory:")
    try:
        conn.execute("CREATE VIRTUAL TABLE s USING fts5(c, tokenize='unicode61')")
        conn.execute("CREATE VIRTUAL TABLE sv USING fts5vocab('s', 'instance')")
        conn.executemany("INSERT INTO s(rowid, c) VALUES (?, ?)", list(enumerate(texts)))
        out = [[] for _ in texts]
        for term, doc, _ in conn.execute("SELECT term, doc, offset FROM sv ORDER BY doc, offset"):
            out[doc].append(term)
        return out
    finally:
        conn.close()


# the mix of the random strings: ASCII, the marks, Latin / Greek / Cyrillic letters, CJK, full-width forms, emoji, punctuation
_POOLS = None


def _pools(model: Model):
    global _POOLS
    if _POOLS is None:
        marks = [cp for cp in range(2 * T.UNICODE_PLANE) if model.cls[cp] == T.UNICODE_MARK]
        _POOLS = [
            [ord(c) for c in "abcXYZ019 .,-_'\t"],
            marks,
            list(range(0xC0, 0x250)) + list(range(0x370, 0x400)) + list(range(0x400, 0x530)) + [0x23A, 0x2C65, 0x1E9E, 0x212A],
            list(range(0x4E00, 0x4E40)) + list(range(0x3040, 0x3100)) + list(range(0xAC00, 0xAC20)),
            list(range(0xFF01, 0xFF5F)),
            list(range(0x1F600, 0x1F640)) + list(range(0x10400, 0x10450)) + list(range(0x1D400, 0x1D440)),
            [0xA0, 0xAD, 0xB7, 0x2013, 0x2014, 0x2026, 0x200B, 0x200D, 0x3000, 0x0483, 0x05B0, 0x093C, 0x20D0, 0xFE0F],
        ]
    return _POOLS


def random_strings(n: int, seed: int, model: Model, max_len: int = 30):
    rng = random.Random(seed)
    pools = _pools(model)
    weights = [6, 3, 5, 2, 2, 1, 2]
    out = []
    for _ in range(n):
        k = rng.randint(0, max_len)
        out.append("".join(chr(rng.choice(rng.choices(pools, weights)[0])) for _ in range(k)))
    return out
