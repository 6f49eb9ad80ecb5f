"""Two independent restatements of the text matcher, shared by the CPU and GPU tests:

  ast_search(ast, text)      a position-set simulation straight on the parsed AST over code points -- no NFA, no UTF-8, no
                             subset construction: what the pipeline of next_plaid_amd/regexes.py must agree with;
  run_packed(words, strings) an interpreter of the exact packed table that crosses the ABI (include/nextplaid_hip.h): what the
                             device must agree with bit for bit.
"""
import numpy as np

ACCEPT_AT_END, MATCHED, DEAD = 1, 2, 4
_WORD = set(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ_abcdefghijklmnopqrstuvwxyz")


def _is_word(text, i):
    return 0 <= i < len(text) and ord(text[i]) in _WORD


def _assert(kind, text, i):
    if kind == "bol":
        return i == 0
    if kind == "eol":
        return i == len(text)
    if kind == "mbol":
        return i == 0 or text[i - 1] == "\n"
    if kind == "meol":
        return i == len(text) or text[i] == "\n"
    boundary = _is_word(text, i - 1) != _is_word(text, i)
    return boundary if kind == "wb" else not boundary


def _ends(node, text, starts):
    """the positions a match of `node` can end at when it starts at one of `starts`"""
    k = node[0]
    if k == "set":
        out = set()
        for i in starts:
            if i < len(text):
                c = ord(text[i])
                if any(lo <= c <= hi for lo, hi in node[1]):
                    out.add(i + 1)
        return out
    if k == "cat":
        for n in node[1]:
            starts = _ends(n, text, starts)
            if not starts:
                break
        return starts
    if k == "alt":
        out = set()
        for n in node[1]:
            out |= _ends(n, text, starts)
        return out
    if k == "rep":
        _, body, lo, hi = node
        cur = set(starts)
        for _ in range(lo):
            cur = _ends(body, text, cur)
            if not cur:
                return cur
        out, frontier, n = set(cur), cur, lo
        while frontier and (hi is None or n < hi):
            frontier = _ends(body, text, frontier) - out
            out |= frontier
            n += 1
        return out
    return {i for i in starts if _assert(node[1], text, i)}


def ast_search(ast, text: str) -> bool:
    """unanchored is_match"""
    return bool(_ends(ast, text, set(range(len(text) + 1))))


def unpack(words):
    """(start, class_of u8[256], table u16[ns][nc], flags u8[ns]) of packed u32 / i64 words"""
    w = np.ascontiguousarray(np.asarray(words).astype(np.uint32))
    assert w[0] == 0x4146444E
    ns, nc = int(w[1]), int(w[2])
    f0 = 68
    t0 = f0 + (ns + 3) // 4
    assert w.size == t0 + (ns * nc + 1) // 2
    return (int(w[3]), w[4:68].view(np.uint8), w[t0:].view(np.uint16)[:ns * nc].reshape(ns, nc), w[f0:t0].view(np.uint8)[:ns])


def run_packed(words, strings) -> np.ndarray:
    """bool [len(strings)]: the walk of every byte string through the packed table, as the header defines it"""
    start, class_of, table, flags = unpack(words)
    cls, tab, fl = class_of.tolist(), table.tolist(), flags.tolist()
    out = np.zeros(len(strings), bool)
    for j, s in enumerate(strings):
        st = start
        for b in s:
            if fl[st] & (MATCHED | DEAD):
                break
            st = tab[st][cls[b]]
        out[j] = bool(fl[st] & ACCEPT_AT_END)
    return out


def select(prog, schema, lo: int = 0, hi=None) -> np.ndarray:
    """tests/filter_restate.py's select for a program that may hold NP_F_MATCH leaves: each is restated as the IN list of the
    codes whose dictionary string the packed table accepts (an IN list without a NULL has MATCH's three values: TRUE on a match,
    UNKNOWN on a NULL cell, FALSE otherwise), and the rest of the program is evaluated as before."""
    import filter_restate as FR
    from next_plaid_amd import filters as F
    cols = sorted(schema.columns.values(), key=lambda c: c.index)
    ops, values = [], list(prog.values.tolist())
    for op, ci, arg, nv, first in prog.ops:
        if op == F.NP_F_MATCH:
            codes = np.flatnonzero(run_packed(prog.values[first:first + nv], cols[ci].dictionary)).tolist()
            ops.append((F.NP_F_IN, ci, 0, len(codes), len(values)))
            values += codes
        else:
            ops.append((op, ci, arg, nv, first))
    return FR.select(F.CompiledFilter(ops, np.array(values, np.int64).reshape(-1)), schema, lo, hi)


def bits_of(verdicts: np.ndarray) -> np.ndarray:
    """bool [n] -> u32 [ceil(n / 32)], bit s of word s / 32"""
    n = verdicts.size
    padded = np.zeros((n + 31) // 32 * 32, np.uint8)
    padded[:n] = verdicts
    return np.packbits(padded, bitorder="little").view("<u4").copy()
