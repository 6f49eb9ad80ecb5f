"""The table generators of tests/regex_restate.py that tests/test_gpu_match_limits.py drives the device with, checked without a
device: each builds a regexes.Dfa the ABI check accepts, the counter's closed form and the vectorised interpreter equal
run_packed (the definition), the rolling verdicts split the strings, the absorbing variants stop where they are planted, and the
extreme tables pack to the word counts np_match_plan.h expects.  The kernel's walk is restated too (tile_walk_model), with one
line wrong at a time, to show on the device tests' own inputs that a byte lost or doubled at a tile boundary, a state mask of
11 bits and a tile index counted from the unaligned base each change the bits those tests compare."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from next_plaid_amd import regexes as R
import regex_restate as RR

MAX_STRING_BYTES = 4 << 20   # NP_MATCH_MAX_STRING_BYTES


def random_strings(n, seed, lo=0, hi=600):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, int(k)).astype(np.uint8).tobytes() for k in rng.integers(lo, hi + 1, n)]


def well_formed(d):
    """what match_check_dfa asks of a table, restated"""
    ns, nc = d.table.shape
    assert 1 <= ns <= R.DFA_MAX_STATES and 1 <= nc <= R.DFA_MAX_CLASSES and 0 <= d.start < ns
    assert d.class_of.dtype == np.uint8 and d.class_of.shape == (256,) and int(d.class_of.max()) < nc
    assert d.table.dtype == np.uint16 and int(d.table.max()) < ns and d.flags.dtype == np.uint8 and d.flags.shape == (ns,)
    assert not (d.flags & ~np.uint8(R.ACCEPT_AT_END | R.MATCHED | R.DEAD)).any()
    for s in np.flatnonzero(d.flags & (R.MATCHED | R.DEAD)):
        assert (d.table[s] == s).all()
        assert bool(d.flags[s] & R.MATCHED) == bool(d.flags[s] & R.ACCEPT_AT_END) and bool(d.flags[s] & R.DEAD) != bool(d.flags[s] & R.MATCHED)
    w = d.pack()
    assert w.dtype == np.uint32 and w.size == RR.dfa_words(ns, nc)
    back = R.Dfa.unpack(w)
    assert back.start == d.start and np.array_equal(back.class_of, d.class_of) and np.array_equal(back.table, d.table) and \
        np.array_equal(back.flags, d.flags) and np.array_equal(back.pack(), w)
    return w


GENERATED = {
    "counter-251x3": lambda: RR.counter(251, 3, {0, 7, 250}),
    "counter-7x1": lambda: RR.counter(7, 1, {3}),
    "counter-64x4-start-60": lambda: RR.counter(64, 4, {37}, start=60),
    "rolling-61x256": lambda: RR.rolling(61, 256, 3),
    "rolling-4093x256": lambda: RR.rolling(4093, 256, 5),
    "rolling-13x5": lambda: RR.rolling(13, 5, 2),
    "absorbing-counter": lambda: RR.absorbing(RR.counter(251, 3, {0, 7, 250}), (17, 1), (40, 2)),
    "absorbing-rolling": lambda: RR.absorbing(RR.rolling(61, 256, 3), (5, 9), (33, 200)),
}


@pytest.mark.parametrize("name", sorted(GENERATED))
def test_generated_tables_are_well_formed_and_both_interpreters_agree(name):
    d = GENERATED[name]()
    w = well_formed(d)
    strings = random_strings(300, 11) + [b"", b"\x00", b"\xff" * 97]
    want = RR.run_packed(w, strings)
    assert np.array_equal(RR.run_packed_np(w, strings), want)
    assert np.array_equal(RR.run_packed_np(w, strings, short=0), want) and np.array_equal(RR.run_packed_np(w, strings, short=1000), want)
    assert np.array_equal(RR.run_packed_np(w.astype(np.int64), strings[:40]), want[:40])      # as a filter's values hold it
    assert 0 < int(want.sum()) < len(strings), name                                          # neither all true nor all false
    if name.startswith("absorbing"):
        stops = [RR.stops_at(w, s) for s in strings]
        assert d.flags[-2:].tolist() == [R.ACCEPT_AT_END | R.MATCHED, R.DEAD]
        assert any(x is not None for x in stops) and sum(x is None for x in stops) > 10         # both kinds of walk
    else:
        assert not (d.flags & (R.MATCHED | R.DEAD)).any()


def test_counter_closed_form_equals_the_walk():
    strings = random_strings(400, 5)
    lens = [len(s) for s in strings]
    for ns, nc, accept, start in ((251, 3, {0, 7, 250}, 0), (7, 1, {3}, 0), (64, 4, {37}, 60), (4096, 2, {2048, 4095}, 0), (4096, 1, {0}, 4095), (1, 256, {0}, 0)):
        d = RR.counter(ns, nc, accept, start)
        assert (d.table == ((np.arange(ns) + 1) % ns)[:, None]).all() and set(np.flatnonzero(d.flags).tolist()) == set(accept)
        want = RR.run_packed(d.pack(), strings)
        assert np.array_equal(RR.counter_verdicts(ns, accept, lens, start), want), (ns, nc)
    # one byte more or fewer flips the verdict of a counter with a single accepting state
    assert RR.counter_verdicts(4096, {0}, [MAX_STRING_BYTES - 1, MAX_STRING_BYTES, MAX_STRING_BYTES + 1]).tolist() == [False, True, False]
    assert MAX_STRING_BYTES % 4096 == 0


def test_rolling_depends_on_every_byte_and_on_their_order():
    d = RR.rolling(4093, 256, 5)
    assert sorted(d.class_of.tolist()) == list(range(256)) and not np.array_equal(d.class_of, np.arange(256))
    assert d.table[4092, 255] == (4092 * 3 + 256) % 4093 and int(d.table.max()) == 4092 and (d.flags[::5] == R.ACCEPT_AT_END).all()
    rng = np.random.default_rng(3)
    s = rng.integers(0, 256, 300).astype(np.uint8)
    end = RR.state_after(d, s.tobytes())
    for at in (0, 1, 150, 298, 299):
        dropped, doubled, swapped = np.delete(s, at), np.insert(s, at, s[at]), s.copy()
        other = (at + 1) % 300
        swapped[[at, other]] = swapped[[other, at]]
        changed = s.copy()
        changed[at] ^= 0x10
        for t in (dropped, doubled, changed) + ((swapped,) if s[at] != s[other] else ()):
            assert RR.state_after(d, t.tobytes()) != end, at
    small = RR.rolling(61, 256, 3)
    assert small.table.nbytes == 31232 and RR.image_bytes(61, 256) - 256 == 31232


def test_absorbing_variants_stop_at_the_planted_byte():
    base = RR.rolling(61, 256, 3)
    rng = np.random.default_rng(9)
    c_m, c_d = 77, 78
    free = np.array([b for b in range(256) if base.class_of[b] not in (c_m, c_d)], np.uint8)
    byte_of = {int(c): b for b, c in enumerate(base.class_of.tolist())}
    for k in (0, 1, 500):
        prefix = free[rng.integers(0, free.size, k)].tobytes()
        tail = rng.integers(0, 256, 40).astype(np.uint8).tobytes()
        st = RR.state_after(base, prefix)
        other = (st + 1) % 61
        hit = RR.absorbing(base, (st, c_m), (other, c_d))
        dead = RR.absorbing(base, (other, c_m), (st, c_d))
        well_formed(hit), well_formed(dead)
        s_m, s_d = prefix + bytes([byte_of[c_m]]) + tail, prefix + bytes([byte_of[c_d]]) + tail
        assert RR.stops_at(hit.pack(), s_m) == k and RR.stops_at(dead.pack(), s_d) == k
        assert RR.run_packed(hit.pack(), [s_m, s_d, prefix]).tolist()[:1] == [True]
        assert RR.run_packed(dead.pack(), [s_d]).tolist() == [False]
        assert RR.stops_at(base.pack(), s_m) is None


# ---- what the device tests would notice: the kernel's walk restated, with one line wrong at a time --------------------------

def differs(words, strings, tile, defect, want=None):
    want = RR.run_packed(words, strings) if want is None else want
    assert np.array_equal(RR.tile_walk_model(words, strings, tile), want)          # the restated walk itself is right
    return not np.array_equal(RR.tile_walk_model(words, strings, tile, defect), want)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_boundary_strings_notice_a_byte_lost_or_doubled_at_a_tile_boundary(order):
    """The strings of test_gpu_match_limits' first test at a tile of 64 bytes: a position one too far or one short when a lane
    leaves a tile flips bits under every table, plain and absorbing, in every order and for every planted position."""
    T = 64
    rng = np.random.default_rng(17)
    lens = RR.boundary_lengths(T, order, rng)
    plain = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lens]
    bases = RR.walk_tables(lens)
    for defect in ("skip", "repeat"):
        seen = [differs(base.pack(), plain, T, defect) for base in bases]
        assert seen[1] and (seen[2] or seen[3]), (defect, seen)             # the alternating counter always, a rolling hash
    for where in RR.PLANTS:
        strings, at = RR.plant(plain, T, where, rng)
        (i_m, _), (i_d, _) = at.items()
        dfas = [RR.absorbing_at(base, strings, at) for base in bases]
        for defect in ("skip", "repeat"):
            seen = []
            for d in dfas:
                want = RR.run_packed(d.pack(), strings)
                assert want[i_m] and not want[i_d]
                seen.append(differs(d.pack(), strings, T, defect, want))
            assert any(seen), (where, defect, seen)   # (a counter that absorbs re-enters its pair every 251 bytes: often blind)
    # the closed form of the longest string: 256 tiles walked once end in state 0 of counter(4096, 1), any other count does not
    long = [bytes(5), bytes(256 * T), bytes(3)]
    w = RR.counter(4096, 1, {0}).pack()
    want = RR.counter_verdicts(4096, {0}, [len(s) for s in long])
    assert want.tolist() == [False, True, False] and differs(w, long, T, "skip", want) and differs(w, long, T, "repeat", want)


def test_high_states_notice_a_narrow_state_mask():
    rng = np.random.default_rng(31)
    lens = [4094, 4095, 4096, 8191, 2047, 2048, 0, 1, 6]
    strings = [rng.integers(0, 256, n).astype(np.uint8).tobytes() for n in lens]
    for d, acc, start in ((RR.counter(4096, 256, {4095}), {4095}, 0), (RR.counter(4096, 2, {2048, 4095}), {2048, 4095}, 0),
                          (RR.counter(4096, 4, {4095, 3}, start=4095), {4095, 3}, 4095)):
        assert differs(d.pack(), strings, 16384, "mask", RR.counter_verdicts(4096, acc, lens, start))
    short = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(0, 41, 600)]
    assert differs(RR.rolling(4093, 256, 5).pack(), short, 16384, "mask")
    assert not differs(RR.rolling(61, 256, 3).pack(), short, 16384, "mask")       # 61 states never reach the cut bit


def test_residue_sweep_notices_an_index_from_the_unaligned_base():
    """A second block that starts at a byte offset that is no multiple of 16 sees the defect; one that starts on a multiple
    cannot, which is why the sweep takes every residue."""
    rng = np.random.default_rng(60)
    w = RR.rolling(61, 256, 3).pack()
    for r in range(16):
        first = [rng.integers(0, 256, int(k)).astype(np.uint8).tobytes() for k in rng.integers(0, 13, 256)]
        first[-1] += bytes((r - sum(len(s) for s in first)) % 16)
        rest = [rng.integers(0, 256, int(k)).astype(np.uint8).tobytes() for k in rng.integers(1, 13, 200)]
        assert differs(w, first + rest, 16384, "base") == (r != 0), r


@pytest.mark.parametrize("ns,nc", [(4096, 256), (4096, 4), (4096, 5), (4093, 256), (2049, 8), (1, 1), (3, 3)])
def test_extreme_tables_pack_to_the_planned_word_counts(ns, nc):
    d = RR.counter(ns, nc, {ns - 1}) if ns != 4093 else RR.rolling(4093, 256, 5)
    w = d.pack()
    assert w.size == 68 + -(-ns // 4) + -(-(ns * nc) // 2) == RR.dfa_words(ns, nc)
    assert w[0] == R.DFA_MAGIC and (int(w[1]), int(w[2]), int(w[3])) == (ns, nc, 0)
    start, class_of, table, flags = RR.unpack(w)
    assert table.shape == (ns, nc) and np.array_equal(table, d.table) and np.array_equal(flags, d.flags) and np.array_equal(class_of, d.class_of)
    # the sizes the LDS decision of the plan turns on
    sizes = {(4096, 4): 32768, (2049, 8): 32784, (4096, 5): 40960, (4096, 256): 2097152}
    if (ns, nc) in sizes:
        assert RR.image_bytes(ns, nc) - 256 == sizes[(ns, nc)]


def test_word_counts_and_image_sizes_equal_the_plan_header(tmp_path):
    """dfa_words and image_bytes restate match_dfa_words and match_check_dfa's image size: compiled against np_match_plan.h."""
    src = tmp_path / "sizes.cpp"
    src.write_text("""
#include "np_match_plan.h"
int main() {
  const int shapes[][2] = {{4096, 256}, {4096, 4}, {4096, 5}, {4093, 256}, {2049, 8}, {2561, 8}, {1, 1}, {63, 256}, {253, 3}};
  for (auto& s : shapes) {
    np::MatchDfaInfo info;
    const uint32_t h[4] = {NP_DFA_MAGIC, (uint32_t)s[0], (uint32_t)s[1], 0};
    info = np::match_checked_info(h);
    printf("%d %d %lld %lld\\n", s[0], s[1], (long long)np::match_dfa_words(s[0], s[1]), (long long)info.image_bytes);
  }
  printf("%d %d %d %lld %lld\\n", (int)np::NP_MATCH_TILE_BYTES, (int)np::NP_MATCH_LDS_TABLE_BYTES, (int)np::NP_MATCH_LDS_TABLE_MAX,
         (long long)np::NP_MATCH_BLOCK_STRINGS, (long long)NP_MATCH_MAX_STRING_BYTES);
  return 0;
}
""")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "next-plaid_amd", "csrc"),
                           str(src), "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    for line in lines[:9]:
        ns, nc, words, image = map(int, line.split())
        assert words == RR.dfa_words(ns, nc) and image == RR.image_bytes(ns, nc), line
    assert list(map(int, lines[9].split())) == [16384, 32768, 40960, 256, MAX_STRING_BYTES]
