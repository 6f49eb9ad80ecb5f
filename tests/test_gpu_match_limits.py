"""np_hip_text_match and the NP_F_MATCH leaf at the match kernel's own limits, bit for bit against the interpreter of the packed
table (tests/regex_restate.py: run_packed, its vectorised twin run_packed_np, and the counter's closed form where a text is too
long for a Python loop).  The tables are generated, not compiled: a counter and a rolling hash whose verdict changes with
every byte walked, so a byte lost or doubled at a tile boundary, a state number cut by a wrong mask, a table on the wrong side
of the LDS budget, an output row of another DFA, a misaligned staging base or a bitmap that is a word short all flip bits.
tests/test_match_limits_cpu.py checks the generators without a device.  Needs a real MI355X."""
import threading

import numpy as np
import pytest

from helpers import hip_index, make_arrays

import next_plaid_amd as npa
from next_plaid_amd import regexes as R
import regex_restate as RR

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

N_DOCS = 900
BLOCK = 256                     # NP_MATCH_BLOCK_STRINGS
MAX_STRING_BYTES = 4 << 20      # NP_MATCH_MAX_STRING_BYTES
GROUP_MAX = 4096 // 24          # MATCH_GROUP_MAX: descriptors of 24 bytes in the 4096 bytes behind a group's images
F = npa.filters


def up256(v):
    return (v + 255) & ~255


@pytest.fixture(scope="module")
def handle():
    """One small index; column 0 ("s") holds code 0 in every row, so any dictionary of at least one string may be set as its
    text, in any order, through np_hip_index_set_column_text itself."""
    spec, a = make_arrays(num_docs=N_DOCS, num_centroids=32, dim=32, nbits=2, doc_len_min=2, doc_len_max=6, seed=21)
    hx = hip_index(a)
    hx.set_columns({"s": ["x"] * N_DOCS})
    hx.set_column_text_raw(0, [b"x"])
    hx.text_match_raw(0, [R.compile_regex("x", True).pack()], 1)
    tile = hx.last_match_report["tile_bytes"]
    assert tile >= 64 and tile % 16 == 0 and MAX_STRING_BYTES == 256 * tile
    yield spec, a, hx, tile
    hx.close()


def match(hx, strings, dfas, what="", want=None):
    """the device's bits over the text the column holds == the interpreter's (or `want`, one bool row per DFA, where a closed
    form stands in for it); returns them and the report"""
    packed = [d.pack() if isinstance(d, R.Dfa) else d for d in dfas]
    got = hx.text_match_raw(0, packed, len(strings))
    rep = dict(hx.last_match_report)
    assert got.dtype == np.uint32 and got.shape == (len(packed), (len(strings) + 31) // 32)
    for j, w in enumerate(packed):
        exp = RR.bits_of(np.asarray(want[j], bool) if want is not None else RR.run_packed_np(w, strings))
        assert np.array_equal(got[j], exp), f"{what}: DFA {j}: strings {np.flatnonzero(np.unpackbits((got[j] ^ exp).view(np.uint8), bitorder='little'))[:8]} differ"
    assert rep["bytes_scanned"] == sum(len(s) for s in strings) * len(packed)
    assert rep["n_lds"] + rep["n_global"] == len(packed)
    return got, rep


def check(hx, strings, dfas, what="", want=None):
    hx.set_column_text_raw(0, strings)
    return match(hx, strings, dfas, what, want)


def random_bytes(rng, n):
    return rng.integers(0, 256, int(n)).astype(np.uint8).tobytes()


def short_random(n, seed, hi=40):
    rng = np.random.default_rng(seed)
    return [random_bytes(rng, k) for k in rng.integers(0, hi + 1, n)]


def bit_count(bits):
    return int(np.unpackbits(bits.view(np.uint8)).sum())


# ---- 1: every byte walked once, in order ------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_every_byte_is_walked_once_and_in_order(handle, order):
    """One block whose strings start and end before, on and after tile boundaries.  The plain tables' verdicts change with
    every byte and (rolling) with their order.  The absorbing variants enter MATCHED in the longest string and DEAD in the
    2T + 1 one at a known byte: the last byte of a tile, the first byte of the next one, and the string's byte 0; before that
    byte those strings hold no byte of the entering class, so the walk cannot stop earlier (RR.plant, RR.absorbing_at)."""
    spec, a, hx, T = handle
    rng = np.random.default_rng(17)
    lens = RR.boundary_lengths(T, order, rng)
    bases = RR.walk_tables(lens)
    assert bases[2].table.nbytes == 31232
    plain = [random_bytes(rng, n) for n in lens]
    _, rep = check(hx, plain, bases, f"{order}: plain")
    assert (rep["n_lds"], rep["n_global"], rep["n_chunks"]) == (3, 1, 1)
    for where in RR.PLANTS:
        strings, at = RR.plant(plain, T, where, rng)
        (i_m, _), (i_d, _) = at.items()
        dfas = [RR.absorbing_at(base, strings, at) for base in bases]
        got, rep = check(hx, strings, dfas + (bases if where == "byte 0" else []), f"{order}: absorbing at the {where}")
        for j in range(len(dfas)):
            assert (got[j, 0] >> i_m) & 1 == 1 and (got[j, 0] >> i_d) & 1 == 0
        assert rep["n_global"] == (2 if where == "byte 0" else 1)


# ---- 2: the longest string ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_text():
    rng = np.random.default_rng(23)
    return random_bytes(rng, MAX_STRING_BYTES), short_random(300, 24)


# one lane's walk of NP_MATCH_MAX_STRING_BYTES was measured once (profiles/match_time.md): 0.56 s a call, 0.6 s the test; the
# limit is about three times that, on the test itself (the handle's set-up is not the walk)
@pytest.mark.timeout(2, func_only=True)
@pytest.mark.parametrize("place", ["first in its block", "last in its block"])
def test_the_longest_string_is_walked_to_its_last_byte(handle, long_text, place):
    """A string of exactly NP_MATCH_MAX_STRING_BYTES, 256 tiles, among 300 short ones: the first string of the second block,
    then the last of the first.  counter(4096, 1, {0}) accepts it iff all 4 194 304 bytes were walked once; {1} rejects it.  The
    expected bits are the closed form (no Python loop over 4 MiB)."""
    spec, a, hx, T = handle
    long, short = long_text
    at = BLOCK if place[0] == "f" else BLOCK - 1
    strings = short[:at] + [long] + short[at:]
    lens = [len(s) for s in strings]
    assert len(long) == MAX_STRING_BYTES == 256 * T and len(strings) == 301 and MAX_STRING_BYTES % 4096 == 0
    accept = [{0}, {1}, {4095, 7}]
    want = [RR.counter_verdicts(4096, acc, lens) for acc in accept]
    assert want[0][at] and not want[1][at] and not want[2][at]
    hx.set_column_text_raw(0, strings)
    got, rep = match(hx, strings, [RR.counter(4096, 1, acc) for acc in accept], place, want)
    print(f"{place}: the 256-tile walk, three counters: {rep['ms']:.1f} ms")
    assert rep["n_lds"] == 3 and rep["n_chunks"] == 1
    # MATCHED at byte 10 of the long string: its block stops staging long before the text ends.  Bits only, not the time.
    base = RR.counter(4000, 2, {3, 9})
    c10 = int(base.class_of[long[10]])
    d = RR.absorbing(base, (10, c10), (12, 1 - int(base.class_of[long[12]])))
    head = long[:64]
    assert RR.stops_at(d.pack(), head) == 10
    want = RR.run_packed_np(d.pack(), short[:at] + [head] + short[at:])   # the verdict is decided inside the head
    assert want[at]
    _, rep = match(hx, strings, [d], place + ", MATCHED at byte 10", [want])
    print(f"{place}: MATCHED at byte 10: {rep['ms']:.2f} ms")


# ---- 3: the state field -----------------------------------------------------------------------------------------------------

def test_state_numbers_up_to_4095_on_both_table_paths(handle):
    spec, a, hx, T = handle
    rng = np.random.default_rng(31)
    lens = [4094, 4095, 4096, 8191, 2047, 2048, 0, 1, 6]
    strings = [random_bytes(rng, n) for n in lens]
    wide, narrow = RR.counter(4096, 256, {4095}), RR.counter(4096, 2, {2048, 4095})
    from_top = [RR.counter(4096, 4, {4095, 3}, start=4095), RR.counter(4096, 256, {4095, 3}, start=4095)]
    dfas = [wide, narrow] + from_top
    want = [RR.counter_verdicts(4096, {4095}, lens), RR.counter_verdicts(4096, {2048, 4095}, lens),
            RR.counter_verdicts(4096, {4095, 3}, lens, 4095), RR.counter_verdicts(4096, {4095, 3}, lens, 4095)]
    assert want[0].tolist() == [False, True, False, True, False, False, False, False, False]
    assert want[1].tolist() == [False, True, False, True, False, True, False, False, False]     # ends in 4094 4095 0 4095 2047 2048 0 1 6
    assert want[2].tolist() == [False, False, True, False, False, False, True, False, False] and lens[6] == 0   # 4095 + 4096, 4095 + 0
    got, rep = check(hx, strings, dfas, "counters of 4096 states", want)
    assert (rep["n_lds"], rep["n_global"]) == (2, 2)
    again, _ = check(hx, strings, dfas, "counters of 4096 states, by the interpreter")
    assert np.array_equal(got, again)
    lens4 = [4, 4100, 8196, 5, 4095]                                 # from state 4095: 4 bytes later the walk is in state 3
    strings4 = [random_bytes(rng, n) for n in lens4]
    want4 = [RR.counter_verdicts(4096, {4095, 3}, lens4, 4095)] * 2
    assert want4[0].tolist() == [True, True, True, False, False]
    check(hx, strings4, from_top, "start state 4095", want4)
    # every state of a 4093-state table is entered: ~600 short random strings and one longer than a tile
    many = short_random(2 * BLOCK + 88, 32)
    many[7] = random_bytes(rng, T + 77)
    roll = RR.rolling(4093, 256, 5)
    got, rep = check(hx, many, [roll, RR.rolling(4093, 256, 5, start=4092)], "rolling(4093, 256, 5)")
    assert rep["n_global"] == 2 and 0 < bit_count(got[0]) < len(many)
    seen = {RR.state_after(roll, s) for s in many}
    assert max(seen) >= 2048 and sum(s >= 2048 for s in seen) > 100


# ---- 4: the LDS budget edge --------------------------------------------------------------------------------------------------

def test_tables_on_either_side_of_the_lds_budget(handle):
    """A table goes to LDS when its bytes (the image less the 256 class bytes) are at most match_lds KiB.  4096 x 4 is exactly
    32 768 bytes, 2049 x 8 is 16 more; 4096 x 5 is exactly 40 960, the most the knob gives (16 384 + 256 + 40 960 = 57 600 bytes
    of dynamic LDS a block), 2561 x 8 is 16 more.  Every table gives the same bits down both paths."""
    spec, a, hx, T = handle
    rng = np.random.default_rng(41)
    strings = short_random(BLOCK + 60, 42) + [random_bytes(rng, n) for n in (4095, 4096, 5000, T + 77)]
    tables = {32768: RR.rolling(4096, 4, 5), 32784: RR.counter(2049, 8, {2048, 5}), 40960: RR.rolling(4096, 5, 5), 40976: RR.rolling(2561, 8, 5)}
    for size, d in tables.items():
        assert d.table.nbytes == size and RR.image_bytes(d.n_states, d.n_classes) - 256 == size
    hx.set_column_text_raw(0, strings)
    want = {size: [RR.run_packed_np(d.pack(), strings)] for size, d in tables.items()}
    assert all(0 < int(w[0].sum()) < len(strings) for w in want.values())
    bits = {}

    def run(size, path, lds_kib):
        got, rep = match(hx, strings, [tables[size]], f"{size} bytes at match_lds = {lds_kib}", want[size])
        assert (rep["n_lds"], rep["n_global"]) == ((1, 0) if path == "lds" else (0, 1)), (size, lds_kib, rep)
        assert rep["table_lds_bytes"] == min(lds_kib, 40) * 1024
        assert bits.setdefault(size, got.tobytes()) == got.tobytes()

    try:
        for size, path in ((32768, "lds"), (32784, "global"), (40960, "global"), (40976, "global")):
            run(size, path, 32)
        for lds_kib in (40, 41):                                     # the knob is clamped to 40
            hx.tune("match_lds", lds_kib)
            for size, path in ((32768, "lds"), (32784, "lds"), (40960, "lds"), (40976, "global")):
                run(size, path, lds_kib)
        hx.tune("match_lds", 0)
        for size in tables:
            run(size, "global", 0)
    finally:
        hx.tune("match_lds", 32)
    run(32768, "lds", 32)


# ---- 5: groups of DFAs -------------------------------------------------------------------------------------------------------

PRIMES = [5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79]


def small_dfa(j):
    """distinct small tables, counters and rolling hashes in turn"""
    if j % 2:
        n = 2 + j % 37
        return RR.counter(n, 1 + j % 5, {j % n, (3 * j + 1) % n})
    return RR.rolling(PRIMES[(j // 2) % len(PRIMES)], 1 + (j // 2) % 9, 2 + (j // 40) % 3, start=j % 5)


@pytest.fixture(scope="module")
def grouped(handle):
    """2 * 256 + 9 short strings, 341 small tables and two of the global path, and every table's bits when it runs alone"""
    spec, a, hx, T = handle
    strings = short_random(2 * BLOCK + 9, 51, hi=14)
    small = [small_dfa(j) for j in range(2 * GROUP_MAX + 1)]
    assert len({d.key() for d in small}) > 300
    big = [RR.rolling(4093, 256, 5), RR.rolling(4093, 256, 7, start=9)]
    hx.set_column_text_raw(0, strings)
    alone = {}
    for d in small + big:
        got, rep = match(hx, strings, [d], "alone")
        alone[id(d)] = got[0].copy()
        assert rep["n_chunks"] == 1
    assert sum(0 < bit_count(b) < len(strings) for b in alone.values()) > 300
    return strings, small, big, alone


def group_call(grouped, n, at):
    strings, small, big, alone = grouped
    dfas = list(small[:n])
    dfas[at[0]], dfas[at[1]] = big
    return dfas, [np.unpackbits(alone[id(d)].view(np.uint8), bitorder="little")[:len(strings)] for d in dfas]


@pytest.mark.parametrize("n,at,chunks", [(GROUP_MAX, (0, GROUP_MAX - 1), 1), (GROUP_MAX + 1, (GROUP_MAX - 1, GROUP_MAX), 2),
                                         (2 * GROUP_MAX + 1, (0, 2 * GROUP_MAX), 3), (2 * GROUP_MAX + 1, (GROUP_MAX, 2 * GROUP_MAX - 1), 3)])
def test_groups_of_170_dfas_keep_every_row_in_place(handle, grouped, n, at, chunks):
    """A launch group holds at most 170 DFAs; inside it the descriptors are ordered [LDS | global] while every DFA keeps its
    own output row.  Two global-path tables sit at the first and the last slot of a group or alone in a trailing group of one."""
    spec, a, hx, T = handle
    assert GROUP_MAX == 170
    strings = grouped[0]
    hx.set_column_text_raw(0, strings)
    dfas, want = group_call(grouped, n, at)
    got, rep = match(hx, strings, dfas, f"{n} DFAs", want)               # every row == that DFA alone on the device ...
    assert (rep["n_lds"], rep["n_global"], rep["n_chunks"]) == (n - 2, 2, chunks)
    again, _ = match(hx, strings, dfas, f"{n} DFAs, interpreter")         # ... and == the interpreter
    assert np.array_equal(got, again)


def test_groups_times_string_chunks_under_a_tight_workspace(handle, grouped):
    """match_plan (np_match_plan.h): all n DFAs are one planned group when budget >= sum of the images (each rounded up to 256)
    + 4096 + n * 32, and a chunk then holds (budget - sum - 4096) / (n * 32) blocks of strings.  With exactly that budget the
    171 DFAs run one block of 256 strings at a time: 3 string chunks, times the 2 launch groups the cap of 170 makes of them."""
    spec, a, _, T = handle
    strings = grouped[0]
    n = GROUP_MAX + 1
    dfas, want = group_call(grouped, n, (GROUP_MAX - 1, GROUP_MAX))
    images = sum(up256(RR.image_bytes(d.n_states, d.n_classes)) for d in dfas)
    budget = images + 4096 + n * (BLOCK // 8)
    assert (budget - images - 4096) // (n * (BLOCK // 8)) == 1 and images > 2 * 2 * 1024 * 1024
    hx = hip_index(a, workspace_bytes=budget)
    try:
        assert hx.workspace_bytes() == budget
        hx.set_columns({"s": ["x"] * N_DOCS})
        got, rep = check(hx, strings, dfas, "171 DFAs, one block a chunk", want)
        blocks = -(-len(strings) // BLOCK)
        assert blocks == 3 and rep["n_chunks"] == 2 * blocks and (rep["n_lds"], rep["n_global"]) == (n - 2, 2)
    finally:
        hx.close()
    short = hip_index(a, workspace_bytes=budget - 1)                   # one byte less: one DFA at a time, all strings at once
    try:
        short.set_columns({"s": ["x"] * N_DOCS})
        again, rep = check(short, strings, dfas, "171 DFAs, one DFA a group", want)
        assert rep["n_chunks"] == n and np.array_equal(again, got)
    finally:
        short.close()


# ---- 6: alignment ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("r", range(16))
def test_every_pair_of_start_and_end_residues(handle, r):
    """A block stages from off[first] & ~15 up to (B1 + 15) & ~15.  For every q, 256 + 256 + 5 strings whose first 256 end at a
    byte offset = r (mod 16) and whose last ends at = q (mod 16); the sixteen sets of one r share a call, each but the last
    filled up to whole blocks with empty strings so that the next begins a block (at residue q, ending at r: every pair again)."""
    spec, a, hx, T = handle
    rng = np.random.default_rng(60 + r)
    strings, total = [], 0

    def add(n, residue):
        nonlocal total
        part = [random_bytes(rng, k) for k in rng.integers(0, 13, n)]
        end = total + sum(len(s) for s in part)
        part[-1] += random_bytes(rng, (residue - end) % 16)
        strings.extend(part)
        total += sum(len(s) for s in part)
        assert total % 16 == residue

    for q in range(16):
        assert len(strings) % BLOCK == 0
        add(BLOCK, r)
        add(BLOCK, int(rng.integers(0, 16)))
        add(5, q)
        if q < 15:
            strings.extend([b""] * (BLOCK - 5))
    assert len(strings) == 16 * 3 * BLOCK - (BLOCK - 5)
    got, rep = check(hx, strings, [RR.rolling(61, 256, 3), RR.counter(17, 3, {0, 5, 11})], f"r = {r}")
    assert rep["n_lds"] == 2 and 0 < bit_count(got[0]) < len(strings)
    lens = [len(s) for s in strings]
    assert np.array_equal(got[1], RR.bits_of(RR.counter_verdicts(17, {0, 5, 11}, lens)))


# ---- 7: through the filter ---------------------------------------------------------------------------------------------------

FILTER_BLOCK_DOCS = 16384       # NP_FILTER_BLOCK_DOCS
N_FILTER_DOCS = 2 * FILTER_BLOCK_DOCS + 777
TOP = "~" * 37                  # sorts after every other string of its column and is the only one of 37 bytes


def filter_columns():
    rng = np.random.default_rng(71)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz 0123456789"))
    words = set()
    while len(words) < 299:
        words.add("".join(rng.choice(letters, int(rng.integers(1, 31)))))
    a_vals = sorted(words) + [TOP]
    b_vals = a_vals[:9] + a_vals[150:159] + [TOP]                    # 19 strings, all of them also strings of the first column
    a = [a_vals[i] for i in rng.integers(0, 299, N_FILTER_DOCS)]
    b = [b_vals[i] for i in rng.integers(0, len(b_vals), N_FILTER_DOCS)]
    for row in (5, FILTER_BLOCK_DOCS, N_FILTER_DOCS - 1):             # the highest code, in every chunk of documents
        a[row] = TOP
    for row in range(0, N_FILTER_DOCS, 11):
        a[row] = None
    for row in range(3, N_FILTER_DOCS, 7):
        b[row] = None
    return {"a": np.array(a, object), "b": np.array(b, object), "z": np.arange(N_FILTER_DOCS) % 5}, a_vals, b_vals


def match_program(leaves, tail=(), values=None):
    """leaves: (column, packed words) MATCH leaves in order, then the ops of `tail`; values: an array to use as it is"""
    ops, vals = [], []
    for col, w in leaves:
        ops.append((F.NP_F_MATCH, col, 0, int(w.size), sum(v.size for v in vals)))
        vals.append(np.asarray(w).astype(np.int64))
    ops += [(op, -1, 0, 0, 0) for op in tail]
    return F.CompiledFilter(ops, np.concatenate(vals) if values is None else values)


def filter_fixed_bytes(progs, jobs, n_docs):
    """The bytes np_filter.hip plans around: programs (ops of 24 bytes, the op offsets, the constants without the MATCH tables),
    the match passes' bitmaps (whole blocks of 8 words per distinct (column, DFA)) and work area (the largest image + 4096),
    two tables of (filter, document block) totals, and 4096."""
    n_ops = sum(len(p.ops) for p in progs)
    prog = up256(n_ops * 24) + up256((len(progs) + 1) * 4) + up256(8)
    words = sum(-(-n_strings // BLOCK) * (BLOCK // 32) for n_strings, _ in jobs)
    work = max(up256(image) + 4096 for _, image in jobs)
    blocks = -(-n_docs // FILTER_BLOCK_DOCS)
    return prog + up256(words * 4) + up256(work) + 2 * up256((len(progs) * blocks + 1) * 8) + 4096


def test_match_leaves_over_two_columns_through_the_filter():
    """Two CODE columns with text: 300 strings (two blocks of the match kernel, the second partial; not a multiple of 32
    either) and 19.  The highest code of the first is the only string counter(64, 4, {37}) accepts, so its bit is the last one
    of a bitmap's partial block.  Seven bitmaps of two sizes lie behind one another; a table met again, as the same array or as
    equal bytes, shares one."""
    spec, a = make_arrays(num_docs=N_FILTER_DOCS, num_centroids=16, dim=32, nbits=2, doc_len_min=1, doc_len_max=1, seed=3)
    rows, a_vals, b_vals = filter_columns()
    assert len(a_vals) == 300 and len(a_vals) % BLOCK and len(a_vals) % 32 and len(b_vals) < 32
    x, only_top = RR.rolling(61, 256, 3).pack(), RR.counter(64, 4, {37}).pack()
    d1, d2, big = RR.counter(5, 2, {0, 1, 2}).pack(), RR.rolling(13, 5, 2).pack(), RR.rolling(4093, 256, 5).pack()
    shared = match_program([(0, only_top)])
    progs = [match_program([(0, x), (1, x)], [F.NP_F_OR]),                                    # the same table on both columns
             match_program([(0, d1), (0, d2), (0, only_top)], [F.NP_F_AND, F.NP_F_OR]),       # three tables on one column
             match_program([(1, d2), (0, d1), (0, d2)], [F.NP_F_OR, F.NP_F_AND]),
             shared,
             match_program([(0, only_top.copy()), (1, d1)], [F.NP_F_OR]),                     # equal bytes in another array
             match_program([(0, only_top)], values=shared.values),                            # the same array object
             match_program([(0, big)]),                                                       # a global-path table as a leaf
             match_program([(1, d1)], [F.NP_F_NOT]),                                          # NOT over rows with NULLs
             match_program([(0, big), (1, only_top)], [F.NP_F_NOT, F.NP_F_OR])]
    assert progs[5].values is progs[3].values and progs[4].values is not progs[3].values
    # postfix: progs[1] = d1, (d2 AND only_top); progs[2] = d2(b), (d1 OR d2), AND -- the restated select evaluates the same programs
    jobs = [(300, RR.image_bytes(61, 256)), (19, RR.image_bytes(61, 256)), (300, RR.image_bytes(5, 2)), (300, RR.image_bytes(13, 5)),
            (300, RR.image_bytes(64, 4)), (19, RR.image_bytes(13, 5)), (19, RR.image_bytes(5, 2)), (300, RR.image_bytes(4093, 256)),
            (19, RR.image_bytes(64, 4))]
    fixed = filter_fixed_bytes(progs, jobs, N_FILTER_DOCS)
    unit = FILTER_BLOCK_DOCS // 8 + 4 + 8 + 8 * FILTER_BLOCK_DOCS         # filter_block_bytes of a staged (filter, block)
    tight = fixed + len(progs) * unit + unit // 2                          # every filter, one block of documents a chunk: 3 chunks
    results = []
    for budget in (None, tight):
        hx = hip_index(a, **({} if budget is None else {"workspace_bytes": budget}))
        try:
            hx.set_columns(rows, text_on_device=["a", "b"])
            sch = hx.schema
            assert sch["a"].dictionary[-1] == TOP.encode() and len(sch["a"].dictionary) == 300 and len(sch["b"].dictionary) == 19
            if budget is None:
                want = [RR.select(p, sch) for p in progs]
                top_rows = np.flatnonzero((sch["a"].data == 299) & (sch["a"].valid != 0))
                assert np.array_equal(want[3], top_rows) and top_rows.size >= 2 and top_rows[-1] == N_FILTER_DOCS - 1
                assert all(0 < w.size < N_FILTER_DOCS for w in want)
                nulls_b = np.flatnonzero(sch["b"].valid == 0)
                assert nulls_b.size and not np.isin(nulls_b, want[7]).any() and not np.isin(nulls_b, RR.select(match_program([(1, d1)]), sch)).any()
            else:
                assert hx.workspace_bytes() == budget
            runs = [hx.filter_ids(progs)]
            if budget is None:
                hx.tune("match_lds", 0)
                try:
                    runs.append(hx.filter_ids(progs))
                finally:
                    hx.tune("match_lds", 32)
            for got in runs:
                for j, (g, w) in enumerate(zip(got, want)):
                    assert g.dtype == np.int64 and np.array_equal(g, w), f"budget {budget}, filter {j}: {g[:8]} ({g.size}) vs {w[:8]} ({w.size})"
            results += [[g.tobytes() for g in got] for got in runs]
            assert np.array_equal(hx.filter_ids(progs, counts_only=True), [w.size for w in want])
        finally:
            hx.close()
    assert len(results) == 3 and results[0] == results[1] == results[2]


# ---- 8: two threads ----------------------------------------------------------------------------------------------------------

def test_two_threads_match_on_one_handle(handle, grouped):
    spec, a, hx, T = handle
    strings, small, big, alone = grouped
    hx.set_column_text_raw(0, strings)
    lists = [[d.pack() for d in small[:12] + [big[0]] + small[12:20]], [d.pack() for d in small[40:75]]]
    serial = [hx.text_match_raw(0, lst, len(strings)).tobytes() for lst in lists]
    for lst, bits in zip(lists, serial):
        want = np.stack([RR.bits_of(RR.run_packed_np(w, strings)) for w in lst])
        assert bits == want.tobytes()
    out, errs = {}, []

    def work(k):
        try:
            for r in range(4):
                out[(k, r)] = hx.text_match_raw(0, lists[k], len(strings)).tobytes() == serial[k]
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, errs
    assert len(out) == 8 and all(out.values())
