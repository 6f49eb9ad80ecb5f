"""The pattern compilers of next_plaid_amd/regexes.py against three things that share nothing with their NFA -> DFA pipeline:
the position-set simulation on the AST (tests/regex_restate.py), Python's re on the printed translation, and SQLite's own LIKE.

The translation a pattern of the dialect goes through before Python's re sees it (regexes.to_python prints the parsed AST):
  * `$` and `\\z` without m become `\\Z` (Python's `$` also matches before a final newline; the crate's does not);
    `^` without m becomes `\\A`; under m they become the scoped `(?m:^)` and `(?m:$)`;
  * `\\x{...}` and every other literal or class bound becomes `\\xHH`, `\\uHHHH` or `\\UHHHHHHHH`;
  * `(?<n>` and `(?P<n>` lose their name (is_match does not report groups), every group prints as `(?:`;
  * POSIX classes, `\\d \\s \\w` and their negations become ranges;
  * `U` and the lazy suffix are dropped (is_match does not depend on them);
  * flags are resolved per node: a letter under i prints as the class of its case variants, `.` as the class it stands for;
  * `\\B` prints as `(?!\\b)`: Python's `\\B` does not match in the empty string, the crate's does;
  * patterns with Perl classes or `\\b` run under re.ASCII and on ASCII subjects only.
"""
import os
import random
import re
import sqlite3
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from next_plaid_amd import filters as F
from next_plaid_amd import regexes as R
import filter_restate as FR
import regex_restate as RR

# ---- generated patterns ----------------------------------------------------------------------------------------------------

ASCII_SUBJECTS = ["", "\n", "a", "b", "ab", "ba", "abc", "aab", "abab", "\nab", "ab\n", "\nab\n", "a\nb", "a\n\nb", "A", "AB", "aB",
                  "k", "K", "s", "S", "ks", "KS", "a b", " a", "a ", "a_b", "a-b", "a.b", "0", "a0", "0a", "a1b2", "[a]", "a]", "{a}",
                  "a{2}", "^a$", "a|b", "\ta", "a\t", "\r\n", "ab ab", "abcabc", "bbbb", "aaaa", "ba\nab", "zz", "_", "-", "b\nb",
                  "x", "xa", "ax", "a\nx", "x\n", "\nx", "ab\nab\n", "B\nA", "9_9", "..", "a..b",
                  # long mixed subjects: most patterns find something in them
                  "ab0 KS_x\nAb [k]s.", "a b\tks 0_9\nxx AB\n", "k0s Ab\nab{2} ^x$ a|b", "xx aa bb ks KS 00\n_a-b.c/d", "\naA bB kK sS 0_ \n",
                  "s k a b x 0 _ A B K S\n\n", "abab ksks xx00 ABAB\tKSKS", "0a1b2k3s4x5 A_B K-S\n", "ba ab sk ks x0 0x\n\nBA AB",
                  "[a-c] k* s+ x? (ab) {0} \\ / # & ~", "a\nb\nk\ns\nx\n0\nA\nB\nK\nS\n_\n \n"]
WIDE_SUBJECTS = ["é", "aé", "éa", "éé", "É", "ß", "€", "a€b", "€\n", "\n€", "\U0001F600", "a\U0001F600", "\U0001F600b", "K", "ſ",
                 "aK", "ſb", "Kſ", "αβγ", "aα", "α\nβ", "߿ࠀ", "￿\U00010000", "\x7f\x80", "é\n",
                 "\U0010ffff", "kK", "sſ", "日本語", "a日b"]


def _subjects(base, alphabet, count, seed):
    """the named edge cases, then seeded strings over the same alphabet up to `count` distinct subjects"""
    rng = random.Random(seed)
    out, seen = list(base), set(base)
    while len(out) < count:
        s = "".join(rng.choice(alphabet) for _ in range(rng.randint(1, 9)))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


ASCII_ALPHABET = list("aabbABksKSx0_ \n\n.-") + ["\t", "[", "]", "{", "}", "|", "^", "$", "\\", "/", "#", "&", "~", "9", "z", "\r"]
WIDE_ALPHABET = ASCII_ALPHABET + list("é€αß\U0001F600Kſ") + ["É", "日", "߿", "ࠀ", "￿", "\U00010000", "\U0010ffff"]
ASCII_SUBJECTS = _subjects(ASCII_SUBJECTS, ASCII_ALPHABET, 300, 1)
WIDE_SUBJECTS = _subjects(WIDE_SUBJECTS, WIDE_ALPHABET, 200, 2)

PUNCT = ".*+?()[]{}|^$\\-/ #&~"
# every accepted construct, by the name the generator tags it with; each must be in at least five generated patterns
CONSTRUCTS = (["lit:char", "lit:wide", "lit:\\xHH", "lit:\\x{}", "lit:\\x{}wide", "dot", "dot:s", "alternation", "alt:empty-branch",
               "class:range", "class:single", "class:negated", "class:widerange", "class:dash-edge", "class:leading-]", "class:\\xHH-bound",
               "group:(", "group:(?:", "group:(?P<n>", "group:(?<n>", "group:(?flags:", "flags:(?flags)", "flag:i", "flag:m", "flag:s",
               "flag:U", "flag:negated", "quant:*", "quant:+", "quant:?", "quant:{n}", "quant:{n,}", "quant:{n,m}", "quant:lazy",
               "anchor:^", "anchor:$", "anchor:\\A", "anchor:\\z", "anchor:\\b", "anchor:\\B", "anchor:^:m", "anchor:$:m"]
              + ["lit:\\" + c for c in PUNCT] + ["lit:\\" + c for c in "nrtfv"] + ["class:\\" + c for c in "nrtfv"]
              + ["perl:\\" + c for c in "dswDSW"] + ["class:\\" + c for c in "dswDSW"] + ["class:[:" + n + ":]" for n in sorted(R._POSIX)])


def _generator(seed):
    rng = random.Random(seed)
    used = {}       # occurrences so far: choices inside a family go to the least used member
    cur = set()     # the constructs of the pattern being generated

    def tag(t):
        used[t] = used.get(t, 0) + 1
        cur.add(t)

    def least(prefix, options):
        lo = min(used.get(prefix + o, 0) for o in options)
        return rng.choice([o for o in options if used.get(prefix + o, 0) == lo])

    def lit(wide):
        k = rng.choice(["char", "char", "char", "punct", "nrtfv", "\\xHH", "\\x{}"] + (["wide", "\\x{}wide"] if wide else []))
        if k == "char":
            tag("lit:char")
            return rng.choice("abABksKSx0_ ")
        if k in ("punct", "nrtfv"):
            c = least("lit:\\", PUNCT if k == "punct" else "nrtfv")
            tag("lit:\\" + c)
            return "\\" + c
        tag("lit:" + k)
        if k == "\\xHH":
            return "\\x" + rng.choice(["61", "0a", "7F", "5b"])
        if k == "\\x{}":
            return "\\x{" + rng.choice(["62", "0062", "A"]) + "}"
        if k == "wide":
            return rng.choice("é€α\U0001F600ß")
        return "\\x{" + rng.choice(["e9", "20AC", "1F600", "10FFFF", "7ff", "800"]) + "}"

    def klass(wide, perl):
        neg = rng.random() < 0.3
        items = []
        for _ in range(rng.randint(1, 3)):
            k = rng.choice(["range", "single", "posix", "posix", "esc"] + (["perl", "perl"] if perl else []) + (["widerange"] if wide else []))
            if k == "range":
                r = rng.choice(["a-c", "A-K", "0-9", "j-t", "\\x61-\\x{7a}", "!-/"])
                tag("class:\\xHH-bound" if "\\x" in r else "class:range")
                items.append(r)
            elif k == "single":
                tag("class:single")
                items.append(rng.choice(["a", "b", "k", "S", "_", ".", "^" if items else "x", "&", "~", "\\]", "\\-", "\\\\"]))
            elif k == "posix":
                n = least("class:[:", [n + ":]" for n in sorted(R._POSIX)])
                tag("class:[:" + n)
                items.append("[:" + n)
            elif k == "esc":
                c = least("class:\\", "nrtfv")
                tag("class:\\" + c)
                items.append("\\" + c)
            elif k == "perl":
                c = least("class:\\", "dswDSW")
                tag("class:\\" + c)
                items.append("\\" + c)
            else:
                tag("class:widerange")
                items.append(rng.choice(["à-ÿ", "α-ω", "\\x{800}-\\x{FFFF}", "\\x{10000}-\\x{10FFFF}", "\\x{80}-\\x{7ff}", "a-\\x{20AC}"]))
        if neg:
            tag("class:negated")
        if rng.random() < 0.1:
            tag("class:dash-edge")
            items.append("-")
        if rng.random() < 0.06:
            tag("class:leading-]")
            items.insert(0, "]")
        return "[" + ("^" if neg else "") + "".join(items) + "]"

    def atom(depth, wide, perl, fl):
        r = rng.random()
        if depth > 0 and r < 0.25:
            k = rng.choice(["(", "(?:", "(?P<n>", "(?<n>", "(?flags:"])
            tag("group:" + k)
            inner = dict(fl)
            if k == "(?flags:":
                k = "(?" + flags(inner) + ":"
            return k.replace("n>", "g%d>" % rng.randint(0, 99999)) + alt(depth - 1, wide, perl, inner) + ")"
        if r < 0.4:
            return klass(wide, perl)
        if r < 0.5:
            tag("dot:s" if fl["s"] else "dot")
            return "."
        if r < 0.58 and perl:
            c = least("perl:\\", "dswDSW")
            tag("perl:\\" + c)
            return "\\" + c
        return lit(wide)

    def flags(fl):
        """a flag string; updates fl, the generator's own view of the flags in force (for the tags that depend on them)"""
        on = "".join(rng.sample("imsU", rng.randint(1, 2)))
        off = "".join(rng.sample([c for c in "imsU" if c not in on], rng.randint(0, 1)))
        for c in on:
            tag("flag:" + c)
            fl[c] = True
        for c in off:
            fl[c] = False
        if off:
            tag("flag:negated")
        return on + ("-" + off if off else "")

    def piece(depth, wide, perl, fl):
        r = rng.random()
        if r < 0.16:
            k = rng.choice(["^", "$", "\\A", "\\z"] + (["\\b", "\\B"] if perl else []))
            tag("anchor:" + k + (":m" if k in "^$" and fl["m"] else ""))
            return k
        a = atom(depth, wide, perl, fl)
        if rng.random() < 0.4:
            q = rng.choice(["*", "+", "?", "{2}", "{1,}", "{0,2}", "{1,3}"])
            tag("quant:" + ("{n}" if q == "{2}" else "{n,}" if q == "{1,}" else "{n,m}" if q[0] == "{" else q))
            if rng.random() < 0.25:
                tag("quant:lazy")
                q += "?"
            return a + q
        return a

    def cat(depth, wide, perl, fl):
        out = []
        for _ in range(rng.randint(0 if rng.random() < 0.1 else 1, 3)):
            if rng.random() < 0.1:
                tag("flags:(?flags)")
                out.append("(?" + flags(fl) + ")")     # for the rest of the enclosing group, later branches included
            out.append(piece(depth, wide, perl, fl))
        if not out:
            tag("alt:empty-branch")
        return "".join(out)

    def alt(depth, wide, perl, fl):
        n = 1 if rng.random() < 0.6 else rng.randint(2, 3)
        if n > 1:
            tag("alternation")
        return "|".join(cat(depth, wide, perl, fl) for _ in range(n))

    def one(ascii_only):
        cur.clear()
        before = dict(used)
        pat = alt(2, not ascii_only, ascii_only, {"i": False, "m": False, "s": False, "U": False})
        return pat, set(cur), lambda: (used.clear(), used.update(before))

    return one


def generated_patterns():
    """(pattern, ascii_only) pairs, and for every construct the number of generated PATTERNS that hold it.  A pattern the
    compiler refuses for a stated reason that depends on context (a non-ASCII literal that ends up under an inline (?i), two
    class items that read as a set operation, too many states) is generated again."""
    one = _generator(20240607)
    rng = random.Random(7)
    out, holds = [], {}
    while len(out) < 360:
        ascii_only = rng.random() < 0.55
        pat, constructs, undo = one(ascii_only)
        try:
            R.compile_regex(pat, ascii_only, max_states=1500)
        except R.FilterError as e:
            assert any(why in str(e) for why in ("(?i)", "max_states", "set operation", "duplicate group name")), (pat, str(e))
            undo()
            continue
        out.append((pat, ascii_only))
        for c in constructs:
            holds[c] = holds.get(c, 0) + 1
    # the empty pattern is one pattern, not a construct that can recur: it is checked once over each kind of column
    return out + [("", True), ("", False)], holds


@pytest.fixture(scope="module")
def generated():
    return generated_patterns()


def test_generated_patterns_agree_three_ways(generated):
    pats, holds = generated
    assert len(pats) >= 300 and len(ASCII_SUBJECTS) >= 300 and len(WIDE_SUBJECTS) >= 200
    assert len(set(ASCII_SUBJECTS)) == len(ASCII_SUBJECTS) and all(s.isascii() for s in ASCII_SUBJECTS)
    rare = {c: holds.get(c, 0) for c in CONSTRUCTS if holds.get(c, 0) < 5}
    assert not rare, f"constructs in fewer than five generated patterns: {rare}"
    assert not set(holds) - set(CONSTRUCTS), set(holds) - set(CONSTRUCTS)
    n_match = n_pairs = 0
    for pat, ascii_only in pats:
        ast = R.parse_regex(pat, ascii_only)
        subjects = ASCII_SUBJECTS if ascii_only else ASCII_SUBJECTS + WIDE_SUBJECTS
        words = R.compile_ast(ast).pack()
        got = RR.run_packed(words, [s.encode("utf-8") for s in subjects])
        py = re.compile(R.to_python(ast), re.ASCII)
        for s, g in zip(subjects, got):
            a = RR.ast_search(ast, s)
            p = py.search(s) is not None
            assert g == a == p, f"{pat!r} (ascii_only={ascii_only}) on {s!r}: DFA {g}, AST {a}, re {p} ({py.pattern!r})"
            n_match += int(g)
            n_pairs += 1
    assert n_match * 3 >= n_pairs and (n_pairs - n_match) * 3 >= n_pairs, (n_match, n_pairs)


def test_meanings_kept_exact():
    def m(pat, s, ascii_only=False):
        return bool(RR.run_packed(R.compile_regex(pat, ascii_only).pack(), [s.encode()])[0])
    assert m("a$", "a") and not m("a$", "a\n") and m("(?m)a$", "a\n") and m("(?m)a$", "a\nb") and not m("(?m)a$", "ab")
    assert m("(?m)^b", "a\nb") and not m("^b", "a\nb") and m("(?m)^$", "a\n") and m("\\Aa\\z", "a") and not m("\\Aa\\z", "a\n")
    assert m("(?i)k", "K") and m("(?i)s", "ſ") and m("(?i)[^k]", "k") is False and not m("(?i)[^k]", "K")
    assert not m("(?i)k", "K".encode().decode()[:0] + "x") and m("(?i)K", "k", True)
    assert m(".", "é") and not m("^.$", "\n") and m("(?s)^.$", "\n") and not m("^.$", "éé") and m("^..$", "éé")
    assert m("", "") and m("", "x") and m("a|", "zzz") and m("\\B", "", True) and not m("\\b", "", True)
    assert m("\\bab\\b", "x ab y", True) and not m("\\bab\\b", "xab y", True) and m("a\\B", "ab", True)
    d = R.compile_regex("", True)
    assert d.n_states == 1 and d.flags[0] == (R.ACCEPT_AT_END | R.MATCHED)
    d = R.compile_regex("[^\\x00-\\x{10FFFF}]", False)
    assert d.n_states == 1 and d.flags[0] == R.DEAD


REFUSED = [
    ("a(?=b)", "lookaround"), ("a(?!b)", "lookaround"), ("(?<=a)b", "lookaround"), ("(?<!a)b", "lookaround"), ("(a)\\1", "backreference"),
    ("(?>a)", "atomic"), ("a*+", "possessive"), ("a++", "possessive"), ("a?+", "possessive"), ("\\pL", "\\p"), ("\\PL", "\\P"),
    ("[\\p{L}]", "\\p"), ("[a&&b]", "&&"), ("[a--b]", "--"), ("[a~~b]", "~~"), ("[a[b]]", "unescaped '['"), ("\\<a", "\\<"), ("a\\>", "\\>"),
    ("\\b{start}", "\\b{"), ("\\Ga", "\\G"), ("a\\K", "\\K"), ("a\\Z", "\\Z"), ("\\C", "\\C"), ("\\07", "octal"), ("[\\101]", "octal"),
    ("(?x)a b", "flag x"), ("(?R)a", "flag R"), ("(?u)a", "flag u"), ("(?-u:a)", "flag u"), ("a{,3}", "{,n}"), ("a{", "escape it"),
    ("a{x}", "escape it"), ("a}", "escape it"), ("{2}", "escape it"), ("a**", "quantifier applied to a quantifier"),
    ("a{2}{3}", "quantifier applied to a quantifier"), ("a*?*", "quantifier applied to a quantifier"), ("^*", "applied to an anchor"),
    ("\\b+", "applied to an anchor"), ("$?", "applied to an anchor"), ("(?i)é", "non-ASCII literal under (?i)"),
    ("(?i)[à-ÿ]", "non-ASCII class bound under (?i)"), ("\\e", "\\e"), ("(?P<a>x)(?<a>y)", "duplicate group name"), ("(", "unclosed"), ("a)", "unmatched"), ("[a", "unclosed class"),
]


@pytest.mark.parametrize("pattern,names", REFUSED)
def test_refused_by_name(pattern, names):
    with pytest.raises(R.FilterError) as e:
        R.compile_regex(pattern, True)
    assert names in str(e.value) and "position" in str(e.value), str(e.value)


def test_refused_for_the_column_and_the_size():
    for pat in ("\\d", "\\S", "[\\w]", "a\\b", "\\B"):
        R.compile_regex(pat, True)
        with pytest.raises(R.FilterError, match="ASCII"):
            R.compile_regex(pat, False)
    with pytest.raises(R.FilterError, match=r"code 17 is not ASCII"):
        R.compile_regex("\\w", False, first_non_ascii=17)
    with pytest.raises(R.FilterError, match=r"max_states = 4096 DFA states \(\d+ reached\)"):
        R.compile_regex("(a|b)*a(a|b){12}", True)
    with pytest.raises(R.FilterError, match=r"max_states = 50"):
        R.compile_regex("(a|b)*a(a|b){6}", True, max_states=50)
    assert R.compile_regex("(a|b)*a(a|b){6}", True).n_states > 50


# ---- LIKE against SQLite itself --------------------------------------------------------------------------------------------

LIKE_STRINGS = sorted(set(
    ["", "a", "A", "ab", "AB", "aB", "abc", "a_c", "a%c", "%", "_", "%%", "__", "\n", "a\n", "\na", "a\nb", "é", "É", "éa", "aé", "Éa", "émile",
     "Émile", "EMILE", "emile", "ß", "SS", "ss", "ſ", "s", "K", "k", "K", "€", "a€", "€a", "a€c", "€€", "\U0001F600", "a\U0001F600",
     "\U0001F600a", "日本", "日本語", "a日c", "α", "Α", "αβ", "ΑΒ", "%é", "_é", "é%", "é_", "a%é_c", " ", "a b", "abcabc", "cab", "bca"]
    + [a + b + c for a in "aé%" for b in "b€_\n" for c in ("", "c", "É")]
    + ["x" * n for n in (1, 2, 3, 7)] + ["é" * n for n in (2, 3)]
    + ["".join(_r.choice(["a", "A", "b", "c", "é", "É", "€", "\U0001F600", "日", "%", "_", "\n", "s", "K", " ", "x", "α", "Α"])
               for _ in range(_r.randint(1, 6))) for _r in [random.Random(9)] for _ in range(200)]))


def like_patterns(count=300, seed=3):
    rng = random.Random(seed)
    alphabet = ["a", "A", "b", "c", "B", "é", "É", "€", "\U0001F600", "日", "%", "%", "_", "_", "\n", "s", "k", "K", " ", "x", "α", "Α", "ß"]
    out = ["", "%", "_", "%%", "%_", "_%", "__", "%é%", "_é", "é_", "%\n%", "a%", "%a", "A_C", "é%", "É%", "%€_", "_\U0001F600", "x%x%x"]
    while len(out) < count:
        out.append("".join(rng.choice(alphabet) for _ in range(rng.randint(1, 5))))
    return out


def test_like_equals_sqlite_on_every_row():
    assert len(LIKE_STRINGS) >= 200
    con = sqlite3.connect(":memory:")
    con.execute("CREATE TABLE t (id INTEGER PRIMARY KEY, s TEXT)")
    con.executemany("INSERT INTO t VALUES (?, ?)", list(enumerate(LIKE_STRINGS)))
    raw = [s.encode("utf-8") for s in LIKE_STRINGS]
    pats = like_patterns()
    assert len(pats) >= 300
    hits = 0
    for p in pats:
        want = np.zeros(len(raw), bool)
        want[[r[0] for r in con.execute("SELECT id FROM t WHERE s LIKE ?", [p])]] = True
        got = RR.run_packed(R.compile_like(p).pack(), raw)
        assert np.array_equal(got, want), f"LIKE {p!r}: differs on {[LIKE_STRINGS[i] for i in np.flatnonzero(got != want)]}"
        hits += int(want.sum())
    assert hits > len(pats)


# ---- the marked schema against today's host path ---------------------------------------------------------------------------

def test_marked_schema_selects_what_the_host_path_selects():
    rows = FR.make_rows(400, seed=5)
    plain = F.make_schema(rows, 400)
    marked = F.make_schema(rows, 400, text_on_device=("s", "t"))
    assert marked["t"].first_non_ascii is not None and marked["s"].text_on_device and not plain["s"].text_on_device
    con = FR.sqlite_table(rows)
    conds = [("t LIKE ?", ["%a%"]), ("NOT (t LIKE ?)", ["al%"]), ("s LIKE ? OR t LIKE ?", ["a_c", "%é"]), ("s LIKE ? AND y > ?", ["AB%", 0]),
             ("NOT (s LIKE ?) AND NOT (t LIKE ?)", ["%b%", "%_x"]), ("t LIKE ? OR y IS NULL", ["É%"]), ("s LIKE ?", [None]),
             ("NOT (s LIKE ?)", [None]), ("s LIKE ? OR z = ?", [None, 1]), ("t LIKE ? AND x < ?", ["%", 0.5]), ("t LIKE ?", [""]),
             ("NOT (t LIKE ? OR s LIKE ?)", ["%z9", "abc_"]), ("s LIKE ?", ["émile"]), ("t NOT IN (?, ?) AND t LIKE ?", ["alpha", "Beta", "%a"])]
    for cond, params in conds:
        a = F.compile_filter(cond, params, plain)
        b = F.compile_filter(cond, params, marked)
        assert not any(o[0] == F.NP_F_MATCH for o in a.ops)
        if any(p is not None for p in params if isinstance(p, (str, type(None)))) and "LIKE" in cond and None not in params:
            assert any(o[0] == F.NP_F_MATCH for o in b.ops), cond
        want = FR.select(a, plain)
        assert np.array_equal(RR.select(b, marked), want), cond
        assert np.array_equal(FR.sqlite_ids(con, cond, params), want), cond
    # REGEXP has no host path to compare with: the per-string truth is Python's re on patterns both dialects share
    for cond, params, rx in [("t REGEXP ?", ["^al"], "^al"), ("t NOT REGEXP ?", ["a$"], None), ("NOT (s REGEXP ?) OR z = ?", ["b", 1], None),
                             ("s REGEXP ? AND t REGEXP ?", ["(?i)^ab", "é|z9"], None), ("s REGEXP ?", [None], None),
                             ("s NOT REGEXP ?", [None], None)]:
        prog = F.compile_filter(cond, params, marked)
        got = RR.select(prog, marked)
        if params[0] is None:
            assert prog.ops[0][0] == F.NP_F_CONST and got.size == 0
            continue
        t = np.array([None if v is np.ma.masked else v for v in rows["t"]], object)
        s = np.array([None if v is np.ma.masked else v for v in rows["s"]], object)
        z = np.asarray(rows["z"])
        if cond == "t REGEXP ?":
            want = [i for i in range(400) if t[i] is not None and re.search(rx, t[i])]
        elif cond == "t NOT REGEXP ?":
            want = [i for i in range(400) if t[i] is not None and not re.search("a\\Z", t[i])]   # a NULL cell stays UNKNOWN
        elif cond.startswith("NOT"):
            want = [i for i in range(400) if (s[i] is not None and "b" not in s[i]) or z[i] == 1]
        else:
            want = [i for i in range(400) if s[i] is not None and t[i] is not None and re.search("^ab", s[i], re.I) and re.search("é|z9", t[i])]
        assert got.tolist() == want, cond
    with pytest.raises(F.FilterError, match="REGEXP.*text_on_device"):
        F.compile_filter("s REGEXP ?", ["a"], plain)
    with pytest.raises(F.FilterError, match="REGEXP"):
        F.compile_filter("s NOT REGEXP ?", ["a"], plain)
    with pytest.raises(F.FilterError, match="type mismatch"):
        F.compile_filter("s REGEXP ?", [3], marked)
    with pytest.raises(F.FilterError, match="code \\d+ is not ASCII"):
        F.compile_filter("t REGEXP ?", ["\\w+"], marked)
    with pytest.raises(F.FilterError, match="row 2.*not UTF-8"):
        F.make_schema({"s": np.array([b"a", b"b", b"\xff\xfe"], object)}, 3, text_on_device=("s",))
    # a marked column whose cells are all NULL has an empty dictionary and no text to keep: UNKNOWN everywhere, no MATCH leaf
    empty = F.make_schema({"e": np.ma.MaskedArray(np.array(["a", "b", "c"]), [True, True, True])}, 3, text_on_device=("e",))
    assert empty["e"].dictionary == [] and empty["e"].text_on_device
    for cond in ("e REGEXP ?", "e NOT REGEXP ?", "e LIKE ?"):
        prog = F.compile_filter(cond, ["a"], empty)
        assert prog.ops[0][:3] == (F.NP_F_CONST, -1, F.CONST_UNKNOWN) and RR.select(prog, empty).size == 0
    with pytest.raises(F.FilterError, match="not a text column"):
        F.make_schema({"y": np.arange(3)}, 3, text_on_device=("y",))


# ---- the stand-alone plan check ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sanitize", [False, True])
def test_match_plan_check_program(tmp_path, sanitize):
    exe = str(tmp_path / "match_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "next-plaid_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "match_plan_check.cpp"),
           "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(cmd)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "match plan check ok" in r.stdout
