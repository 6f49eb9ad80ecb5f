"""The keyword-index build (np_hip_text_build) restated in plain Python: what SQLite's FTS5 makes of ASCII text, the rule
that sends a document to the fallback list, fts5vocab's (term, doc, pos) order and the merge of the fallback documents'
instances.  tests/test_textbuild_restate_cpu.py pins it to SQLite itself; the GPU tests compare the device with SQLite
directly and use this only to say where they differ.

The rules (SQLite 3.37, pure-ASCII text):
  unicode61  token characters are [0-9A-Za-z]; every other byte 0x00..0x7F separates, NUL included; A-Z fold to a-z; a
             token's position is its ordinal in the document, from 0
  trigram    (no NUL in the text) every byte offset i <= len - 3 is a token: lower(bytes[i:i+3]) at position i
  order      terms by memcmp, the shorter string first on a tie (Python's bytes order); inside a term by (doc, pos)
  n_rows     every inserted row counts, empty ones too

`defect` plants one wrong rule, to show that the comparison with SQLite catches it."""
import numpy as np

MAX_TOKEN_BYTES = 256
DEFECTS = ("nul_token", "underscore_token", "no_fold", "byte_pos", "longer_first", "unstable_sort", "nrows_nonempty",
           "trigram_past_end")


def is_token_byte(c: int, defect=None) -> bool:
    if defect == "nul_token" and c == 0:
        return True
    if defect == "underscore_token" and c == 0x5F:
        return True
    return 0x30 <= c <= 0x39 or 0x41 <= c <= 0x5A or 0x61 <= c <= 0x7A


def fold(b: bytes, defect=None) -> bytes:
    return b if defect == "no_fold" else b.lower()     # bytes.lower() folds A-Z only


def unicode61_tokens(raw: bytes, defect=None):
    """[(term, position, byte offset, byte length)] of one document."""
    out, i, n = [], 0, len(raw)
    while i < n:
        if is_token_byte(raw[i], defect):
            j = i
            while j < n and is_token_byte(raw[j], defect):
                j += 1
            out.append((fold(raw[i:j], defect), i if defect == "byte_pos" else len(out), i, j - i))
            i = j
        else:
            i += 1
    return out


def trigram_tokens(raw: bytes, defect=None):
    last = len(raw) - 3 + (1 if defect == "trigram_past_end" else 0)
    return [(fold(raw[i:i + 3], defect), i, i, len(raw[i:i + 3])) for i in range(0, last + 1) if raw[i:i + 3]]


def is_fallback(raw: bytes, tokenizer: str, max_token_bytes: int = MAX_TOKEN_BYTES) -> bool:
    """The document is handed back to the host: a byte >= 0x80; trigram: a NUL; unicode61: a token longer than the cap."""
    if any(c >= 0x80 for c in raw):
        return True
    if tokenizer == "trigram":
        return 0 in raw
    return any(t[3] > max_token_bytes for t in unicode61_tokens(raw))


def order(instances, defect=None):
    """(term, doc, pos) tuples in fts5vocab's order."""
    if defect == "longer_first":
        return sorted(instances, key=lambda t: (t[0] + b"\xff" * 64, -len(t[0]), t[1], t[2]))
    if defect == "unstable_sort":     # sorted by term alone, from an input that is not in (doc, pos) order
        return sorted(reversed(instances), key=lambda t: t[0])
    return sorted(instances)


def arrays(instances, n_rows):
    """Sorted (term, doc, pos) tuples -> the arrays of a TextIndexData."""
    terms, starts = [], []
    for i, t in enumerate(instances):
        if not terms or t[0] != terms[-1]:
            terms.append(t[0])
            starts.append(i)
    return dict(terms=terms, term_offsets=np.asarray(starts + [len(instances)], np.int64),
                inst_doc=np.asarray([t[1] for t in instances], np.int64).reshape(-1),
                inst_pos=np.asarray([t[2] for t in instances], np.int32).reshape(-1), n_rows=int(n_rows))


def build(raws, tokenizer: str = "unicode61", max_token_bytes: int = MAX_TOKEN_BYTES, defect=None):
    """What the device returns for the documents it reproduces: the arrays, and fallback_docs (which contribute nothing)."""
    tok = trigram_tokens if tokenizer == "trigram" else unicode61_tokens
    inst, fb = [], []
    for d, raw in enumerate(raws):
        if is_fallback(raw, tokenizer, max_token_bytes):
            fb.append(d)
            continue
        inst += [(t[0], d, t[1]) for t in tok(raw, defect)]
    n_rows = sum(1 for r in raws if r) if defect == "nrows_nonempty" else len(raws)
    out = arrays(order(inst, defect), n_rows)
    out["fallback_docs"] = fb
    return out


def instances_of(a):
    """The (term, doc, pos) tuples of arrays()."""
    out = []
    for t, term in enumerate(a["terms"]):
        for i in range(int(a["term_offsets"][t]), int(a["term_offsets"][t + 1])):
            out.append((term, int(a["inst_doc"][i]), int(a["inst_pos"][i])))
    return out


def merge(a, b):
    """The device's arrays and the fallback documents' (same shape; disjoint documents): one linear merge per term."""
    ia, ib, out = instances_of(a), instances_of(b), []
    i = j = 0
    while i < len(ia) or j < len(ib):
        if j >= len(ib) or (i < len(ia) and ia[i] < ib[j]):
            out.append(ia[i])
            i += 1
        else:
            out.append(ib[j])
            j += 1
    return arrays(out, a["n_rows"])


def restrict(a, docs):
    """The instances of `docs` alone, as arrays (what the host adds for the fallback documents)."""
    keep = set(int(d) for d in docs)
    return arrays([t for t in instances_of(a) if t[1] in keep], a["n_rows"])


def same(a, b) -> bool:
    return (list(a["terms"]) == list(b["terms"]) and np.array_equal(a["term_offsets"], b["term_offsets"])
            and np.array_equal(a["inst_doc"], b["inst_doc"]) and np.array_equal(a["inst_pos"], b["inst_pos"])
            and int(a["n_rows"]) == int(b["n_rows"]))


def of_data(data):
    """A text.TextIndexData as arrays() with byte-string terms."""
    return dict(terms=[t.encode("utf-8") for t in data.terms], term_offsets=np.asarray(data.term_offsets, np.int64),
                inst_doc=np.asarray(data.inst_doc, np.int64), inst_pos=np.asarray(data.inst_pos, np.int32),
                n_rows=int(data.n_rows))


# ---- corpora -----------------------------------------------------------------------------------------------------------------
def edge_corpus_unicode61():
    every = bytes(range(0x80))
    return ["", "", "hello world", "", "   \t\n", "!!!", "one", "a", "A a AA aA Aa", "x" * 40, "ab abc abcd abcde", "00 0z a a10 a9 ab",
            "prefix1234 prefix1235 prefix12", "sixteenbytesaaaa1 sixteenbytesaaaa2 sixteenbytesaaaa", "snake_case-and.dots",
            every.decode("ascii"), "".join(chr(c) + "q" for c in range(0x80)), "a\x00b \x00 c\x00", "tail ", " head", "", ""]


def edge_corpus_trigram():
    ctl = "".join(chr(c) for c in range(1, 0x20))
    return ["", "a", "ab", "abc", "abcd", "abcde", "ABC", "AbCdE", "  a  ", ctl, "a\tb\nc", "abcabcabc", "", "zzz", "~~~ {|}", ""]


def random_ascii(seed: int, n_docs: int, max_len: int, nul: bool = True):
    rng = np.random.default_rng(seed)
    lo = 0 if nul else 1
    out = []
    for _ in range(n_docs):
        n = int(rng.integers(0, max_len + 1))
        kind = int(rng.integers(0, 3))
        if kind == 0:     # any byte
            b = rng.integers(lo, 0x80, n)
        elif kind == 1:   # words
            b = rng.choice(np.frombuffer(b"abcABC019 _-.\t", np.uint8), n)
        else:             # few letters, many repeats
            b = rng.choice(np.frombuffer(b"ab A", np.uint8), n)
        out.append(bytes(b.astype(np.uint8)).decode("ascii"))
    return out
