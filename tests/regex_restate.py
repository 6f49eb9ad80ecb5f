"""Two independent restatements of the text matcher, shared by the CPU and GPU tests:

  ast_search(ast, text)      a position-set simulation straight on the parsed AST over code points -- no NFA, no UTF-8, no
                             subset construction: what the pipeline of next_plaid_amd/regexes.py must agree with;
  run_packed(words, strings) an interpreter of the exact packed table that crosses the ABI (include/nextplaid_hip.h): what the
                             device must agree with bit for bit;

and, for the tests of the match kernel's limits, run_packed_np (the same walk, short strings side by side in numpy; pinned to
run_packed by tests/test_match_limits_cpu.py) and generated tables: counter, rolling, absorbing.
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


def run_packed_np(words, strings, short=96) -> np.ndarray:
    """run_packed with the strings of at most `short` bytes walked side by side, one numpy step per byte position; the longer
    ones go through the same Python loop.  tests/test_match_limits_cpu.py pins it equal to run_packed, which stays the definition."""
    start, class_of, table, flags = unpack(words)
    lens = np.array([len(s) for s in strings], np.int64)
    state = np.full(len(strings), start, np.int64)
    idx = np.flatnonzero(lens <= short)
    if idx.size and lens[idx].max() > 0:
        ln = lens[idx]
        buf = np.zeros((idx.size, int(ln.max())), np.uint8)
        buf[np.repeat(np.arange(idx.size), ln), np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)] = \
            np.frombuffer(b"".join(strings[i] for i in idx), np.uint8)
        st = state[idx]
        for i in range(buf.shape[1]):
            go = np.flatnonzero((ln > i) & ((flags[st] & (MATCHED | DEAD)) == 0))
            st[go] = table[st[go], class_of[buf[go, i]]]
        state[idx] = st
    rest = np.flatnonzero(lens > short)
    if rest.size:
        cls, tab, fl = class_of.tolist(), table.tolist(), flags.tolist()
    for j in rest:
        st = start
        for b in strings[j]:
            if fl[st] & (MATCHED | DEAD):
                break
            st = tab[st][cls[b]]
        state[j] = st
    return (flags[state] & ACCEPT_AT_END) != 0


def stops_at(words, s: bytes):
    """the index of the byte whose transition enters a MATCHED or DEAD state (-1: the start state is one, None: never)"""
    start, class_of, table, flags = unpack(words)
    cls, tab, fl = class_of.tolist(), table.tolist(), flags.tolist()
    st = start
    if fl[st] & (MATCHED | DEAD):
        return -1
    for i, b in enumerate(s):
        st = tab[st][cls[b]]
        if fl[st] & (MATCHED | DEAD):
            return i
    return None


# ---- tables no compiler would emit, whose verdict depends on every byte (tests/test_gpu_match_limits.py) ---------------------

PERMUTATION = ((np.arange(256) * 167 + 13) % 256).astype(np.uint8)   # an odd multiplier: every class once


def class_map(n_classes):
    """class_of[b] = b % n_classes; with 256 classes a fixed permutation instead (the identity would hide a skipped lookup)"""
    return PERMUTATION.copy() if n_classes == 256 else (np.arange(256) % n_classes).astype(np.uint8)


def counter(n_states, n_classes, accept, start=0):
    """table[s, :] = (s + 1) % n_states, ACCEPT_AT_END exactly on `accept`; no MATCHED or DEAD state.  A string is accepted iff
    (start + len) % n_states is in accept (counter_verdicts): one dropped or doubled byte anywhere flips it."""
    from next_plaid_amd import regexes as R
    table = np.repeat(((np.arange(n_states) + 1) % n_states).astype(np.uint16)[:, None], n_classes, axis=1)
    flags = np.zeros(n_states, np.uint8)
    flags[sorted(accept)] = ACCEPT_AT_END
    return R.Dfa(start, class_map(n_classes), np.ascontiguousarray(table), flags)


def counter_verdicts(n_states, accept, lengths, start=0) -> np.ndarray:
    """the closed form of counter(): needs the lengths only"""
    return np.isin((np.asarray(lengths, np.int64) + start) % n_states, sorted(accept))


def rolling(p, n_classes, accept_mod, start=0):
    """table[s, c] = (3 s + c + 1) % p for a prime p (any p that 3 does not divide will do), ACCEPT_AT_END on the states s % accept_mod == 0: the end state depends on
    every byte and on their order (3 is a unit mod p, so two walks that differ in one byte never meet again by themselves)."""
    from next_plaid_amd import regexes as R
    s, c = np.arange(p, dtype=np.int64)[:, None], np.arange(n_classes, dtype=np.int64)[None, :]
    flags = ((np.arange(p) % accept_mod) == 0).astype(np.uint8) * ACCEPT_AT_END
    return R.Dfa(start, class_map(n_classes), ((s * 3 + c + 1) % p).astype(np.uint16), flags)


def absorbing(d, matched_from, dead_from):
    """`d` with two more states, MATCHED (n_states) and DEAD (n_states + 1), each entered from exactly one (state, class) pair."""
    from next_plaid_amd import regexes as R
    ns, nc = d.table.shape
    table = np.zeros((ns + 2, nc), np.uint16)
    table[:ns] = d.table
    table[ns], table[ns + 1] = ns, ns + 1
    table[matched_from], table[dead_from] = ns, ns + 1
    assert tuple(matched_from) != tuple(dead_from)
    flags = np.concatenate([d.flags, np.array([ACCEPT_AT_END | MATCHED, DEAD], np.uint8)])
    return R.Dfa(d.start, d.class_of.copy(), table, flags)


def state_after(d, s: bytes) -> int:
    """the state of Dfa `d` (no absorbing states) after the bytes of s"""
    cls, tab = d.class_of.tolist(), d.table   # (no list of a 2 MiB table for a short walk)
    st = d.start
    for b in s:
        st = int(tab[st, cls[b]])
    return st


def dfa_words(n_states, n_classes) -> int:
    """words of a packed DFA (match_dfa_words of np_match_plan.h)"""
    return 68 + (n_states + 3) // 4 + (n_states * n_classes + 1) // 2


def image_bytes(n_states, n_classes) -> int:
    """bytes of a DFA's device image: class_of[256] and the u16 table, rounded up to 16 (match_check_dfa's info)"""
    return (256 + n_states * n_classes * 2 + 15) & ~15


# ---- strings around the tile boundaries, and the early exit planted at a known byte -----------------------------------------

BYTE_M, BYTE_D = 100, 200   # the bytes that enter MATCHED / DEAD: classes 1 and 2 of three, two classes of PERMUTATION
FREE = np.array([b for b in range(256) if b % 3 == 0], np.uint8)   # bytes of neither's class under either class map
PLANTS = ("last byte of a tile", "first byte of a tile", "byte 0")


def boundary_lengths(T, order, rng):
    """string lengths before, on and after the boundaries of tiles of T bytes, in the named order"""
    lens = [0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3]
    if order == "descending":
        lens = lens[::-1]
    elif order == "shuffled":
        lens = [lens[i] for i in rng.permutation(len(lens))]
        assert lens != sorted(lens) and lens != sorted(lens)[::-1]
    return lens


def walk_tables(lens):
    """the tables the boundary strings are walked under.  Of these lengths counter(251, 3, {0, 7, 250}) accepts the empty
    string only, and a count that is off by one changes none of its verdicts; the second counter accepts every other length,
    so one byte more or fewer flips any string; the rolling hashes (LDS and global path at the default budget) see the order."""
    alternate = {n % 251 for n in sorted(lens)[::2]}
    assert all((n + d) % 251 in alternate for n in sorted(lens)[::2] for d in (0,)) and \
        not any((n + d) % 251 in alternate for n in sorted(lens)[::2] for d in (-1, 1))
    return [counter(251, 3, {0, 7, 250}), counter(251, 3, alternate), rolling(61, 256, 3), rolling(4093, 256, 5)]


def plant(plain, T, where, rng):
    """`plain` (one block of strings, the first at byte 0 of the text) with the 5T + 3 string rewritten to hold BYTE_M, and the
    2T + 1 string BYTE_D, at the byte that `where` names -- the first tile boundary inside the string, or its byte 0 -- after
    FREE bytes only, so that a table which absorbs on that byte's class cannot stop earlier.  -> strings, {index: byte position}"""
    lens = [len(s) for s in plain]
    off = np.concatenate([[0], np.cumsum(lens)])
    strings, at = list(plain), {}
    for i, byte in ((lens.index(5 * T + 3), BYTE_M), (lens.index(2 * T + 1), BYTE_D)):
        b = int(off[i])
        k = {PLANTS[0]: (b // T + 1) * T - 1 - b, PLANTS[1]: (b // T + 1) * T - b, PLANTS[2]: 0}[where]
        assert 0 <= k < lens[i] and (where == PLANTS[2] or (b + k + (where == PLANTS[0])) % T == 0)
        strings[i] = FREE[rng.integers(0, FREE.size, k)].tobytes() + bytes([byte]) + \
            rng.integers(0, 256, lens[i] - k - 1).astype(np.uint8).tobytes()
        at[i] = k
    return strings, at


def absorbing_at(base, strings, at):
    """`base` with MATCHED entered at the planted byte of the BYTE_M string and DEAD at that of the BYTE_D string (plant)"""
    (i_m, k_m), (i_d, k_d) = at.items()
    assert strings[i_m][k_m] == BYTE_M and strings[i_d][k_d] == BYTE_D
    assert not np.isin(base.class_of[FREE], base.class_of[[BYTE_M, BYTE_D]]).any()
    d = absorbing(base, (state_after(base, strings[i_m][:k_m]), int(base.class_of[BYTE_M])),
                  (state_after(base, strings[i_d][:k_d]), int(base.class_of[BYTE_D])))
    assert stops_at(d.pack(), strings[i_m]) == k_m and stops_at(d.pack(), strings[i_d]) == k_d
    return d


# ---- the kernel's walk restated, to show what a one-line defect would do to the bits (tests/test_match_limits_cpu.py) -------

def tile_walk_model(words, strings, tile, defect=None) -> np.ndarray:
    """match_kernel of np_match.hip in Python: blocks of 256 strings, the text staged tile by tile from a 16-byte aligned base,
    every lane carrying (pos, cur) from tile to tile, table entries of state | flags.  Without a defect it equals run_packed.
    defect: "skip" / "repeat" = pos one too far / one short when a lane leaves a tile unfinished; "mask" = the state taken with
    0x07FF; "base" = the lane's index into the tile counted from off[first] while the tile is staged from off[first] & ~15."""
    start, class_of, table, flags = unpack(words)
    E_STATE, E_ACCEPT, E_DEAD, E_MATCHED = (0x07FF if defect == "mask" else 0x0FFF), 0x2000, 0x4000, 0x8000
    entry = np.arange(flags.size) | np.where(flags & ACCEPT_AT_END, E_ACCEPT, 0) | np.where(flags & DEAD, E_DEAD, 0) | \
        np.where(flags & MATCHED, E_MATCHED, 0)
    nc = table.shape[1]
    tab, cls = entry[table.reshape(-1)].tolist(), class_of.tolist()
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).tolist()
    text = b"".join(strings) + bytes(32)
    out = np.zeros(len(strings), bool)
    for first in range(0, len(strings), 256):
        last = min(first + 256, len(strings))
        B1 = off[last]
        lanes = [[off[s], off[s + 1], int(entry[start])] for s in range(first, last)]   # pos, e, cur
        done = [p >= e or bool(c & (E_MATCHED | E_DEAD)) for p, e, c in lanes]
        t0 = off[first] & ~15
        while t0 < B1 and not all(done):
            n = min(((B1 + 15) & ~15) - t0, tile)
            for j, lane in enumerate(lanes):
                pos, e, cur = lane
                if done[j] or pos >= t0 + n:
                    continue
                iend = min(e, t0 + n) - t0
                i = pos - (off[first] if defect == "base" else t0)
                while i < iend:
                    cur = tab[(cur & E_STATE) * nc + cls[text[t0 + i]]]   # tile[i]
                    i += 1
                    if cur & (E_MATCHED | E_DEAD):
                        break
                pos = t0 + i
                if i == n and pos < e and not cur & (E_MATCHED | E_DEAD):
                    pos += {"skip": 1, "repeat": -1}.get(defect, 0)
                lane[0], lane[2] = pos, cur
                done[j] = pos >= e or bool(cur & (E_MATCHED | E_DEAD))
            t0 += tile
        for j, (pos, e, cur) in enumerate(lanes):
            out[first + j] = bool(cur & E_MATCHED) or (pos >= e and bool(cur & E_ACCEPT))
    return out


def bits_of(verdicts: np.ndarray) -> np.ndarray:
    """bool [n] -> u32 [ceil(n / 32)], bit s of word s / 32"""
    n = verdicts.size
    padded = np.zeros((n + 31) // 32 * 32, np.uint8)
    padded[:n] = verdicts
    return np.packbits(padded, bitorder="little").view("<u4").copy()
