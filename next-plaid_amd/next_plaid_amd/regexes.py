"""REGEXP and LIKE patterns as byte DFAs (the table np_hip_text_match and the NP_F_MATCH filter leaf take).

The crate's REGEXP is the Rust regex crate's is_match (filtering.rs:1969).  A pattern crosses our ABI as a dense DFA over
bytes; this module compiles a STATED dialect of that crate's syntax -- the constructs whose documented meaning this code
reproduces exactly -- and refuses everything else with a FilterError that names the construct and its position.  The pipeline:
parse -> Thompson NFA whose edges are UTF-8 byte ranges -> subset construction -> byte classes -> flags.  The search is
unanchored, so the start state is re-entered at every byte.  Assertions need at most one byte of context on either side: a DFA
state is (NFA states BEFORE their epsilon closure, kind of the previous byte), and the closure is taken when the next byte (or
the end) is known, so `(?m)$` and `\\b` cost no second pass over the text.  Pure host code: no device, no library."""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np

from .api import NextPlaidError

DFA_MAGIC = 0x4146444E
DFA_HEADER_WORDS = 68
DFA_MAX_STATES, DFA_MAX_CLASSES = 4096, 256
ACCEPT_AT_END, MATCHED, DEAD = 1, 2, 4
MAX_CP = 0x10FFFF
_MAX_REPEAT = 1000
_MAX_NFA = 200_000


class FilterError(NextPlaidError):
    """A condition the compiler refuses (the crate's Error::Filtering)."""


# ---- the table -------------------------------------------------------------------------------------------------------

@dataclass
class Dfa:
    """A dense byte DFA: state = table[state, class_of[byte]]; flags per state (ACCEPT_AT_END, MATCHED, DEAD)."""
    start: int
    class_of: np.ndarray   # u8 [256]
    table: np.ndarray      # u16 [n_states, n_classes]
    flags: np.ndarray      # u8 [n_states]

    @property
    def n_states(self):
        return int(self.table.shape[0])

    @property
    def n_classes(self):
        return int(self.table.shape[1])

    def pack(self) -> np.ndarray:
        """The packed words of include/nextplaid_hip.h (u32)."""
        ns, nc = self.table.shape
        fl = np.zeros((ns + 3) // 4 * 4, np.uint8)
        fl[:ns] = self.flags
        tb = np.zeros((ns * nc + 1) // 2 * 2, np.uint16)
        tb[:ns * nc] = self.table.reshape(-1)
        return np.concatenate([np.array([DFA_MAGIC, ns, nc, self.start], np.uint32),
                               np.ascontiguousarray(self.class_of, np.uint8).view("<u4"), fl.view("<u4"), tb.view("<u4")])

    @staticmethod
    def unpack(words) -> "Dfa":
        w = np.ascontiguousarray(words).astype(np.uint32)
        ns, nc = int(w[1]), int(w[2])
        f0 = DFA_HEADER_WORDS
        t0 = f0 + (ns + 3) // 4
        return Dfa(int(w[3]), w[4:68].view(np.uint8).copy(), w[t0:].view(np.uint16)[:ns * nc].reshape(ns, nc).copy(),
                   w[f0:t0].view(np.uint8)[:ns].copy())

    def key(self):
        return self.pack().tobytes()


# ---- sets of scalar values as sorted, disjoint (lo, hi) ranges ------------------------------------------------------------

def _norm(ranges):
    out = []
    for lo, hi in sorted(ranges):
        # surrogates are not scalar values
        for a, b in ((lo, min(hi, 0xD7FF)), (max(lo, 0xE000), hi)):
            if a > b:
                continue
            if out and a <= out[-1][1] + 1:
                out[-1] = (out[-1][0], max(out[-1][1], b))
            else:
                out.append((a, b))
    return out


def _negate(ranges):
    out, at = [], 0
    for lo, hi in _norm(ranges):
        if lo > at:
            out.append((at, lo - 1))
        at = hi + 1
    if at <= MAX_CP:
        out.append((at, MAX_CP))
    return _norm(out)


def _fold(ranges, ascii_only):
    """Simple case folding of ASCII letters; on a non-ASCII column k also matches U+212A and s also matches U+017F."""
    out = list(ranges)
    for lo, hi in ranges:
        for a, z, d in ((0x61, 0x7A, -32), (0x41, 0x5A, 32)):
            x, y = max(lo, a), min(hi, z)
            if x <= y:
                out.append((x + d, y + d))
    out = _norm(out)
    if not ascii_only:
        has = lambda c: any(lo <= c <= hi for lo, hi in out)
        if has(0x6B):
            out.append((0x212A, 0x212A))
        if has(0x73):
            out.append((0x17F, 0x17F))
    return _norm(out)


_DIGIT = [(0x30, 0x39)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_POSIX = {
    "alnum": [(0x30, 0x39), (0x41, 0x5A), (0x61, 0x7A)], "alpha": [(0x41, 0x5A), (0x61, 0x7A)], "ascii": [(0, 0x7F)],
    "blank": [(0x09, 0x09), (0x20, 0x20)], "cntrl": [(0, 0x1F), (0x7F, 0x7F)], "digit": _DIGIT, "graph": [(0x21, 0x7E)],
    "lower": [(0x61, 0x7A)], "print": [(0x20, 0x7E)], "punct": [(0x21, 0x2F), (0x3A, 0x40), (0x5B, 0x60), (0x7B, 0x7E)],
    "space": _SPACE, "upper": [(0x41, 0x5A)], "word": _WORD, "xdigit": [(0x30, 0x39), (0x41, 0x46), (0x61, 0x66)],
}
_PERL = {"d": _DIGIT, "s": _SPACE, "w": _WORD}
_ESC = {"n": 0x0A, "r": 0x0D, "t": 0x09, "f": 0x0C, "v": 0x0B}
_PUNCT = set(" !\"#$%&'()*+,-./:;=?@[\\]^_`{|}~")   # ASCII punctuation and space without < >


# ---- the parser --------------------------------------------------------------------------------------------------------
# AST: ("set", ranges) | ("cat", [nodes]) | ("alt", [nodes]) | ("rep", node, min, max or None) | ("assert", kind), kind in
# bol (\A, ^), eol (\z, $), mbol / meol (^ $ under m), wb (\b), nwb (\B).  Flags are resolved while parsing: a set is already
# folded, a dot already knows about s, an anchor about m.

class _Parser:
    def __init__(self, pat, ascii_only, hint):
        self.p, self.i, self.ascii, self.hint = pat, 0, ascii_only, hint
        self.names = set()

    def fail(self, what, pos=None):
        raise FilterError(f"REGEXP pattern: {what} at position {self.i if pos is None else pos}")

    def peek(self, n=1):
        return self.p[self.i:self.i + n]

    def need_ascii(self, what, pos):
        if not self.ascii:
            self.fail(f"{what} has its ASCII meaning only, and the crate's is Unicode: it is accepted over a column that holds "
                      f"only ASCII{self.hint}; refused", pos)

    def parse(self):
        node = self.alt({"i": False, "m": False, "s": False, "U": False}, 0)
        if self.i < len(self.p):
            self.fail("unmatched ')'")
        return node

    def alt(self, fl, depth):
        fl = dict(fl)   # (?flags) applies to the rest of the enclosing group
        branches, items = [], []
        while self.i < len(self.p) and self.peek() != ")":
            if self.peek() == "|":
                self.i += 1
                branches.append(("cat", items))
                items = []
                continue
            atom = self.atom(fl, depth)
            if atom is None:
                continue
            items.append(self.quantified(atom))
        branches.append(("cat", items))
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def quantified(self, atom):
        c, pos = self.peek(), self.i
        if c not in ("*", "+", "?", "{"):
            if c == "}":
                self.fail("a '}' that closes no counted repetition (escape it: \\})")
            return atom
        if c == "{":
            m = re.compile(r"\{(\d+)(?:(,)(\d*))?\}").match(self.p, self.i)
            if not m:
                if re.compile(r"\{,\d*\}").match(self.p, self.i):
                    self.fail("{,n} (a repetition without a lower count)")
                self.fail("a '{' that is not {n}, {n,} or {n,m} (escape it: \\{)")
            lo = int(m.group(1))
            hi = lo if m.group(2) is None else (None if m.group(3) == "" else int(m.group(3)))
            self.i = m.end()
        else:
            lo, hi = {"*": (0, None), "+": (1, None), "?": (0, 1)}[c]
            self.i += 1
        if atom[0] == "assert":
            self.fail("a quantifier applied to an anchor", pos)
        if hi is not None and hi < lo:
            self.fail("a counted repetition {n,m} with m < n", pos)
        if lo > _MAX_REPEAT or (hi or 0) > _MAX_REPEAT:
            self.fail(f"a repetition count above {_MAX_REPEAT}", pos)
        if self.peek() == "?":   # lazy: is_match does not depend on it
            self.i += 1
        if self.peek() == "+":
            self.fail("a possessive quantifier")
        if self.peek() in ("*", "?", "{") and self.peek() != "":
            self.fail("a quantifier applied to a quantifier")
        return ("rep", atom, lo, hi)

    def lit(self, cp, fl, pos):
        if fl["i"]:
            if cp > 0x7F:
                self.fail("a non-ASCII literal under (?i)", pos)
            return ("set", _fold([(cp, cp)], self.ascii))
        return ("set", _norm([(cp, cp)]))

    def hex_escape(self):
        """after \\x: HH or {H...}"""
        pos = self.i - 2
        if self.peek() == "{":
            m = re.compile(r"\{([0-9A-Fa-f]{1,8})\}").match(self.p, self.i)
            if not m:
                self.fail("a malformed \\x{...} escape", pos)
            self.i = m.end()
            cp = int(m.group(1), 16)
        else:
            m = re.compile(r"[0-9A-Fa-f]{2}").match(self.p, self.i)
            if not m:
                self.fail("a malformed \\xHH escape", pos)
            self.i = m.end()
            cp = int(m.group(0), 16)
        if cp > MAX_CP or 0xD800 <= cp <= 0xDFFF:
            self.fail("a \\x{...} escape that is not a Unicode scalar value", pos)
        return cp

    def escape(self, fl, in_class):
        """after the backslash.  -> ("cp", code point) | ("set", ranges) | ("assert", kind)"""
        pos = self.i - 1
        if self.i >= len(self.p):
            self.fail("a trailing backslash", pos)
        c = self.p[self.i]
        self.i += 1
        if c in _ESC:
            return "cp", _ESC[c]
        if c == "x":
            return "cp", self.hex_escape()
        if c in "dswDSW":
            self.need_ascii(f"\\{c}", pos)
            r = _PERL[c.lower()]
            return "set", (_norm(r) if c.islower() else _negate(r))
        if c in "pP":
            self.fail(f"\\{c} (a Unicode class)", pos)
        if c.isdigit():
            self.fail("an octal escape" if c == "0" or in_class else "a backreference", pos)
        if c in "<>":
            self.fail(f"\\{c} (a word-start / word-end assertion)", pos)
        if not in_class:
            if c in "bB":
                if self.peek() == "{":
                    self.fail("\\b{...}", pos)
                self.need_ascii(f"\\{c}", pos)
                return "assert", "wb" if c == "b" else "nwb"
            if c == "A":
                return "assert", "bol"
            if c == "z":
                return "assert", "eol"
            if c in "GKZC":
                self.fail(f"\\{c}", pos)
        if c in _PUNCT:
            return "cp", ord(c)
        self.fail(f"the escape \\{c}, which is not part of the dialect", pos)

    def atom(self, fl, depth):
        c, pos = self.peek(), self.i
        if c == "(":
            return self.group(fl, depth)
        self.i += 1
        if c == "[":
            return self.klass(fl)
        if c == ".":
            return ("set", _norm([(0, MAX_CP)]) if fl["s"] else _negate([(0x0A, 0x0A)]))
        if c == "^":
            return ("assert", "mbol" if fl["m"] else "bol")
        if c == "$":
            return ("assert", "meol" if fl["m"] else "eol")
        if c == "\\":
            kind, v = self.escape(fl, False)
            if kind == "cp":
                return self.lit(v, fl, pos)
            if kind == "set":
                return ("set", _fold(v, self.ascii) if fl["i"] else v)
            return ("assert", v)
        if c in "*+?":
            self.fail("a quantifier with nothing to repeat", pos)
        if c == "{":
            self.fail("a '{' with nothing to repeat (escape it: \\{)", pos)
        if c == "}":
            self.fail("a '}' that closes no counted repetition (escape it: \\})", pos)
        return self.lit(ord(c), fl, pos)

    def group(self, fl, depth):
        pos = self.i
        self.i += 1
        inner = fl
        if self.peek() == "?":
            self.i += 1
            two, three = self.peek(2), self.peek(3)
            if two in ("P<", ) or (two[:1] == "<" and two not in ("<=", "<!")):
                self.i += 2 if two == "P<" else 1
                m = re.compile(r"[A-Za-z_][A-Za-z0-9_.\[\]]*>").match(self.p, self.i)
                if not m:
                    self.fail("a malformed group name", pos)
                if m.group(0) in self.names:
                    self.fail("a duplicate group name", pos)
                self.names.add(m.group(0))
                self.i = m.end()
            elif two[:1] == ":":
                self.i += 1
            elif two in ("<=", "<!") or two[:1] in ("=", "!"):
                self.fail("lookaround", pos)
            elif two[:1] == ">":
                self.fail("an atomic group", pos)
            elif two == "P=" or three == "P>":
                self.fail("a backreference", pos)
            else:
                on, new, any_flag = True, dict(fl), False
                while True:
                    f = self.peek()
                    if f == "":
                        self.fail("an unclosed group", pos)
                    self.i += 1
                    if f == "-":
                        if not on:
                            self.fail("a doubled '-' in a flag group", pos)
                        on = False
                    elif f in "imsU":
                        new[f] = on
                        any_flag = True
                    elif f in "xRu":
                        self.fail(f"the flag {f}", self.i - 1)
                    elif f in ":)":
                        if not any_flag:
                            self.fail("an empty flag group", pos)
                        break
                    else:
                        self.fail(f"the group syntax (?{f}", pos)
                if f == ")":
                    fl.update(new)   # the rest of the enclosing group
                    return None
                inner = new
        if depth > 200:
            self.fail("groups nested deeper than 200", pos)
        node = self.alt(inner, depth + 1)
        if self.peek() != ")":
            self.fail("an unclosed group", pos)
        self.i += 1
        return node

    def klass(self, fl):
        pos = self.i - 1
        neg = self.peek() == "^"
        if neg:
            self.i += 1
        ranges, first = [], True
        while True:
            if self.i >= len(self.p):
                self.fail("an unclosed class", pos)
            c, at = self.p[self.i], self.i
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if self.peek(2) in ("&&", "--", "~~"):
                self.fail(f"the class set operation {self.peek(2)}")
            if c == "[":
                m = re.compile(r"\[:(\^?)([a-z]+):\]").match(self.p, self.i)
                if not m or m.group(2) not in _POSIX or m.group(1):
                    self.fail("an unescaped '[' inside a class (only [:name:] ASCII classes nest)")
                self.i = m.end()
                ranges += _POSIX[m.group(2)]
                continue
            lo = self.class_bound(fl)
            if lo[0] == "set":
                ranges += lo[1]
                continue
            lo = lo[1]
            hi = lo
            if self.peek() == "-" and self.peek(2) not in ("-]", "--") and self.i + 1 < len(self.p):
                self.i += 1
                if self.peek() == "[":
                    self.fail("an unescaped '[' inside a class (only [:name:] ASCII classes nest)")
                b = self.class_bound(fl)
                if b[0] == "set":
                    self.fail("a class escape as the bound of a range", at)
                hi = b[1]
                if hi < lo:
                    self.fail("a range whose end is below its start", at)
            if fl["i"] and (lo > 0x7F or hi > 0x7F):
                self.fail("a non-ASCII class bound under (?i)", at)
            ranges.append((lo, hi))
        ranges = _norm(ranges)
        if fl["i"]:
            ranges = _fold(ranges, self.ascii)   # fold before negating
        return ("set", _negate(ranges) if neg else ranges)

    def class_bound(self, fl):
        c = self.p[self.i]
        self.i += 1
        if c == "\\":
            return self.escape(fl, True)
        return "cp", ord(c)


def parse_regex(pattern: str, ascii_only: bool, first_non_ascii=None):
    """The pattern as an AST of the dialect (module docstring), or a FilterError naming the construct and its position."""
    if not isinstance(pattern, str):
        raise FilterError("REGEXP pattern: not a string")
    hint = "" if first_non_ascii is None else f" (the string with code {first_non_ascii} is not ASCII)"
    return _Parser(pattern, ascii_only, hint).parse()


def parse_like(pattern: str):
    """SQLite's LIKE as the same AST: % any run of characters, _ one character (a code point), ASCII letters fold and no
    others, no escape character, anchored at both ends."""
    items = [("assert", "bol")]
    everything = _norm([(0, MAX_CP)])
    for ch in pattern:
        if ch == "%":
            items.append(("rep", ("set", everything), 0, None))
        elif ch == "_":
            items.append(("set", everything))
        else:
            items.append(("set", _fold([(ord(ch), ord(ch))], True) if ord(ch) < 0x80 else _norm([(ord(ch), ord(ch))])))
    items.append(("assert", "eol"))
    return ("cat", items)


# ---- printer: the AST as a Python `re` pattern (what the tests compare against) -------------------------------------------

def _pcp(cp):
    return "\\x%02x" % cp if cp < 0x100 else "\\u%04x" % cp if cp < 0x10000 else "\\U%08x" % cp


def to_python(node) -> str:
    """The AST as a pattern Python's re gives the same is_match for: flags are already resolved per node, so no flag is
    needed; \\z and a $ without m print as \\Z, (?m)^ and (?m)$ as scoped (?m:^) and (?m:$), \\B as (?!\\b) (Python's \\B
    does not match the empty string); \\b needs re.ASCII."""
    k = node[0]
    if k == "set":
        if not node[1]:
            return "(?!)"
        return "[" + "".join(_pcp(lo) + ("-" + _pcp(hi) if hi > lo else "") for lo, hi in node[1]) + "]"
    if k == "cat":
        return "".join(to_python(n) for n in node[1])
    if k == "alt":
        return "(?:" + "|".join(to_python(n) for n in node[1]) + ")"
    if k == "rep":
        return "(?:%s){%d,%s}" % (to_python(node[1]), node[2], "" if node[3] is None else node[3])
    return {"bol": "\\A", "eol": "\\Z", "mbol": "(?m:^)", "meol": "(?m:$)", "wb": "\\b", "nwb": "(?!\\b)"}[node[1]]


# ---- NFA over UTF-8 bytes --------------------------------------------------------------------------------------------------

def _utf8(cp):
    if cp < 0x80:
        return [cp]
    if cp < 0x800:
        return [0xC0 | cp >> 6, 0x80 | cp & 0x3F]
    if cp < 0x10000:
        return [0xE0 | cp >> 12, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F]
    return [0xF0 | cp >> 18, 0x80 | cp >> 12 & 0x3F, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F]


def utf8_sequences(lo, hi):
    """A range of scalar values as sequences of byte ranges: the strings the sequences accept are exactly the UTF-8
    encodings of the range."""
    out, stack = [], [(lo, hi)]
    while stack:
        lo, hi = stack.pop()
        for mx in (0x7F, 0x7FF, 0xFFFF):
            if lo <= mx < hi:
                stack += [(mx + 1, hi), (lo, mx)]
                break
        else:
            n = len(_utf8(hi))
            for i in range(1, n):
                m = (1 << 6 * i) - 1
                if lo & ~m != hi & ~m:
                    if lo & m:
                        stack += [((lo | m) + 1, hi), (lo, lo | m)]
                        break
                    if hi & m != m:
                        stack += [(hi & ~m, hi), (lo, (hi & ~m) - 1)]
                        break
            else:
                out.append(tuple(zip(_utf8(lo), _utf8(hi))))
    return out


class _Nfa:
    def __init__(self):
        self.eps, self.byt = [], []
        self.suffix = {}

    def new(self):
        if len(self.eps) >= _MAX_NFA:
            raise FilterError(f"REGEXP pattern: it needs more than {_MAX_NFA} NFA states (counted repetitions multiply)")
        self.eps.append([])
        self.byt.append([])
        return len(self.eps) - 1

    def build(self, node, a):
        k = node[0]
        if k == "set":
            b = self.new()
            for lo, hi in node[1]:
                for seq in utf8_sequences(lo, hi):
                    t = b
                    for j in range(len(seq) - 1, 0, -1):   # shared suffixes: continuation bytes lead to the same end
                        key = (b, seq[j:])
                        s = self.suffix.get(key)
                        if s is None:
                            s = self.suffix[key] = self.new()
                            self.byt[s].append((seq[j][0], seq[j][1], t))
                        t = s
                    self.byt[a].append((seq[0][0], seq[0][1], t))
            return b
        if k == "cat":
            for n in node[1]:
                a = self.build(n, a)
            return a
        if k == "alt":
            b = self.new()
            for n in node[1]:
                s = self.new()
                self.eps[a].append((None, s))
                self.eps[self.build(n, s)].append((None, b))
            return b
        if k == "rep":
            _, body, lo, hi = node
            for _ in range(lo):
                a = self.build(body, a)
            if hi is None:
                loop, s, b = self.new(), self.new(), self.new()
                self.eps[a].append((None, loop))
                self.eps[loop] += [(None, s), (None, b)]
                self.eps[self.build(body, s)].append((None, loop))
                return b
            b = self.new()
            for _ in range(hi - lo):
                self.eps[a].append((None, b))
                a = self.build(body, a)
            self.eps[a].append((None, b))
            return b
        b = self.new()
        self.eps[a].append((node[1], b))
        return b


# kinds of a neighbouring byte
_START, _NL, _WORDB, _OTHER, _END = 0, 1, 2, 3, 4
_IS_WORD = [any(lo <= b <= hi for lo, hi in _WORD) for b in range(256)]


def _kind(b):
    return _NL if b == 0x0A else _WORDB if _IS_WORD[b] else _OTHER


def _holds(cond, prev, nxt):
    if cond == "bol":
        return prev == _START
    if cond == "eol":
        return nxt == _END
    if cond == "mbol":
        return prev in (_START, _NL)
    if cond == "meol":
        return nxt in (_NL, _END)
    same = (prev == _WORDB) == (nxt == _WORDB)
    return not same if cond == "wb" else same


def _asserts(node, out):
    if node[0] == "assert":
        out.add(node[1])
    elif node[0] in ("cat", "alt"):
        for n in node[1]:
            _asserts(n, out)
    elif node[0] == "rep":
        _asserts(node[1], out)
    return out


def compile_ast(ast, max_states: int = DFA_MAX_STATES) -> Dfa:
    """Unanchored is_match of the AST as a Dfa of at most max_states states (FilterError with the count reached otherwise)."""
    max_states = min(int(max_states), DFA_MAX_STATES)
    nfa = _Nfa()
    q0 = nfa.new()
    final = nfa.build(ast, q0)
    used = _asserts(ast, set())
    # the previous byte's kinds that some assertion of the pattern can tell apart; the others fold into _OTHER
    keep = set()
    if used & {"bol", "mbol", "wb", "nwb"}:
        keep.add(_START)
    if "mbol" in used:
        keep.add(_NL)
    if used & {"wb", "nwb"}:
        keep.add(_WORDB)
    red = lambda kd: kd if kd in keep else _OTHER
    # byte classes to step on: between the boundaries of every byte edge and of the kinds
    cuts = {0, 0x0A, 0x0B, 256}
    for lo, hi in _WORD:
        cuts |= {lo, hi + 1}
    for edges in nfa.byt:
        for lo, hi, _ in edges:
            cuts |= {lo, hi + 1}
    cuts = sorted(cuts)
    reps = cuts[:-1]

    closures = {}

    def closure(S, prev, nxt):
        key = (S, prev, nxt)
        got = closures.get(key)
        if got is None:
            seen, stack = set(S), list(S)
            while stack:
                s = stack.pop()
                for cond, t in nfa.eps[s]:
                    if t not in seen and (cond is None or _holds(cond, prev, nxt)):
                        seen.add(t)
                        stack.append(t)
            edges = [e for s in seen for e in nfa.byt[s]]
            got = closures[key] = (final in seen, edges)
        return got

    M, D = -1, -2   # the absorbing states, numbered at the end
    ids = {(frozenset([q0]), red(_START)): 0}
    order = [(frozenset([q0]), red(_START))]
    rows, accept = [], []
    at = 0
    while at < len(order):
        S, prev = order[at]
        at += 1
        accept.append(closure(S, prev, _END)[0])
        row = []
        for r in reps:
            kd = _kind(r)
            hit, edges = closure(S, prev, kd)
            if hit:
                row.append(M)
                continue
            T = frozenset([q0] + [t for lo, hi, t in edges if lo <= r <= hi])
            key = (T, red(kd))
            j = ids.get(key)
            if j is None:
                if len(order) + 2 > max_states:
                    raise FilterError(f"REGEXP pattern: it needs more than max_states = {max_states} DFA states "
                                      f"({len(order) + 2} reached)")
                j = ids[key] = len(order)
                order.append(key)
            row.append(j)
        rows.append(row)
    n = len(rows)
    # states every continuation of which matches fold into MATCHED, states no continuation of which matches into DEAD
    univ = [accept[s] for s in range(n)]
    changed = True
    while changed:
        changed = False
        for s in range(n):
            if univ[s] and any(t != M and not univ[t] for t in rows[s]):
                univ[s] = False
                changed = True
    live = [accept[s] or M in rows[s] for s in range(n)]
    changed = True
    while changed:
        changed = False
        for s in range(n):
            if not live[s] and any(t >= 0 and live[t] for t in rows[s]):
                live[s] = True
                changed = True
    fate = [M if univ[s] else D if not live[s] else s for s in range(n)] + [D, M]   # fate[-1] = M, fate[-2] = D
    # renumber what the start reaches
    start = fate[0]
    new_id, todo = {start: 0}, [start]
    while todo:
        s = todo.pop()
        if s < 0:
            continue
        for t in rows[s]:
            t = fate[t]
            if t not in new_id:
                new_id[t] = len(new_id)
                todo.append(t)
    ns = len(new_id)
    full = np.zeros((ns, len(reps)), np.uint16)
    flags = np.zeros(ns, np.uint8)
    for s, j in new_id.items():
        if s == M:
            full[j, :] = j
            flags[j] = ACCEPT_AT_END | MATCHED
        elif s == D:
            full[j, :] = j
            flags[j] = DEAD
        else:
            full[j, :] = [new_id[fate[t]] for t in rows[s]]
            flags[j] = ACCEPT_AT_END if accept[s] else 0
    # byte classes: step ranges with equal columns
    cols, uniq = {}, []
    class_of = np.zeros(256, np.uint8)
    for c, r in enumerate(reps):
        key = full[:, c].tobytes()
        k = cols.get(key)
        if k is None:
            k = cols[key] = len(uniq)
            uniq.append(c)
        class_of[r:cuts[c + 1]] = k
    return Dfa(0, class_of, np.ascontiguousarray(full[:, uniq]), flags)


def compile_regex(pattern: str, ascii_only: bool, max_states: int = DFA_MAX_STATES, first_non_ascii=None) -> Dfa:
    """`col REGEXP pattern` (unanchored is_match) as a Dfa.  ascii_only = every string the DFA will see is ASCII: \\d \\s \\w
    \\b \\B are accepted only then, and (?i) adds U+212A to k and U+017F to s only otherwise."""
    return compile_ast(parse_regex(pattern, ascii_only, first_non_ascii), max_states)


def compile_like(pattern: str) -> Dfa:
    """`col LIKE pattern` with SQLite's semantics as a Dfa."""
    if isinstance(pattern, bytes):
        try:
            pattern = pattern.decode("utf-8")
        except UnicodeDecodeError as e:
            raise FilterError(f"LIKE pattern is not UTF-8: {e}") from None
    return compile_ast(parse_like(pattern))
