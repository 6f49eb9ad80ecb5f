"""Text predicates on the device: np_hip_index_set_column_text, np_hip_text_match and the NP_F_MATCH filter leaf against the
interpreter of the packed table in tests/regex_restate.py, bit for bit, at the smallest shapes that can break the kernel: string
counts around the ballot word and the block, string lengths around the tile (its size is read from np_match_report), matches
at the first and the last byte and through look-ahead only, both table paths.  Needs a real MI355X."""
import os
import subprocess
import threading

import numpy as np
import pytest

from helpers import ROOT, hip_index, make_arrays, synth

import next_plaid_amd as npa
from next_plaid_amd import regexes as R
from next_plaid_amd import text as T
import filter_restate as FR
import regex_restate as RR
import text_restate as TR

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

N_DOCS = 900
BLOCK = 256


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
    assert tile >= 64 and tile % 16 == 0
    yield spec, a, hx, tile
    hx.close()


def tile_bytes(hx):
    hx.match_text("t", ["a"])
    return hx.last_match_report["tile_bytes"]


def check(hx, strings, dfas, what=""):
    """the device's bits for `strings` as the dictionary of column 0 == the interpreter's; returns them and the report"""
    hx.set_column_text_raw(0, strings)
    packed = [d.pack() if isinstance(d, R.Dfa) else d for d in dfas]
    got = hx.text_match_raw(0, packed, len(strings))
    rep = dict(hx.last_match_report)
    assert got.dtype == np.uint32 and got.shape == (len(packed), (len(strings) + 31) // 32)
    for j, w in enumerate(packed):
        want = RR.bits_of(RR.run_packed(w, strings))
        assert np.array_equal(got[j], want), f"{what}: DFA {j}: strings {np.flatnonzero(np.unpackbits((got[j] ^ want).view(np.uint8), bitorder='little'))[:8]} differ"
    assert rep["bytes_scanned"] == sum(len(s) for s in strings) * len(packed)
    return got, rep


def rx(*patterns, ascii_only=True):
    return [R.compile_regex(p, ascii_only) for p in patterns]


def random_table(n_states, n_classes, seed, absorbing=True):
    """A well-formed table no compiler would emit: random transitions and accepts, optionally a MATCHED and a DEAD state."""
    rng = np.random.default_rng(seed)
    table = rng.integers(0, n_states, (n_states, n_classes)).astype(np.uint16)
    flags = (rng.random(n_states) < 0.4).astype(np.uint8) * R.ACCEPT_AT_END
    if absorbing and n_states >= 4:
        table[(table == 1) | (table == 2)] = 3       # states 1 and 2 absorb: reached from one place each, so most walks go on
        table[0, 0], table[3, 1 % n_classes] = 1, 2
        table[1, :], flags[1] = 1, R.ACCEPT_AT_END | R.MATCHED
        table[2, :], flags[2] = 2, R.DEAD
    class_of = (np.arange(256) % n_classes).astype(np.uint8) if n_classes < 256 else rng.permutation(256).astype(np.uint8)
    return R.Dfa(0, class_of, table, flags)


def short_strings(n, seed):
    rng = np.random.default_rng(seed)
    alphabet = [b"a", b"b", b"\n", b"k", "é".encode(), " ".encode(), b"0"]
    return [b"".join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), int(rng.integers(0, 12)))) for _ in range(n)]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 3 * BLOCK + 37])
def test_string_counts_around_the_word_and_the_block(handle, n):
    spec, a, hx, tile = handle
    dfas = rx("ab", "^b", "a$", "(?m)^a", "(?m)b$", "", "k|\\x{e9}", ascii_only=False) + [R.compile_like("%a_b%"), random_table(9, 5, n)]
    got, rep = check(hx, short_strings(n, n), dfas, f"{n} strings")
    assert 0 < int(np.unpackbits(got.view(np.uint8)).sum()) < n * len(dfas) or n == 1
    assert rep["n_lds"] == len(dfas) and rep["n_global"] == 0 and rep["n_chunks"] == 1
    again, _ = check(hx, short_strings(n, n), dfas)
    assert np.array_equal(got, again)                                # the same bits from run to run


def test_no_strings_is_no_text(handle):
    spec, a, hx, tile = handle
    hx.set_column_text_raw(0, [])                                    # n_strings = 0 drops the text
    with pytest.raises(ValueError, match="no text"):
        hx.text_match_raw(0, [R.compile_regex("a", True).pack()], 1)
    check(hx, [b""], rx("", "a", "^$"))                              # one empty string


def test_lengths_around_the_tile(handle):
    spec, a, hx, T_ = handle
    pats = rx("b", "^b", "b$", "c", "a$", "^$", "(?m)^b", "(?m)a$", "ba", "\\x{1F600}", ascii_only=False)
    lens = [0, 1, T_ - 1, T_, T_ + 1, 3 * T_ + 5]
    fill = lambda n, last=b"": (b"a" * n)[:max(n - len(last), 0)] + last[:n]
    # every length, plain and with the only b at the last byte; in both orders, so each length starts at several offsets
    strings = [fill(n) for n in lens] + [fill(n, b"b") for n in lens]
    check(hx, strings, pats, "ascending lengths")
    check(hx, strings[::-1], pats, "descending lengths")
    check(hx, [b"b" + fill(n - 1) for n in lens if n] + [b""], pats, "the only match at the first byte")
    check(hx, [b""] * 300, rx("", "a", "^$", "(?m)$"), "only empty strings")
    # a string boundary exactly on a tile boundary: string 0 fills tile 0, string 1 starts tile 1, string 2 ends with tile 2
    check(hx, [fill(T_, b"b"), b"b" + fill(T_ - 1), fill(T_ - 1, b"b") + b"a", b"b"], pats, "boundaries on tile boundaries")
    # a 4-byte character straddling the tile boundary at each of its three inner positions
    smile = "\U0001F600".encode()
    for k in (1, 2, 3):
        check(hx, [fill(T_ - k) + smile + b"a", smile, fill(2 * T_ - k) + smile], rx("\\x{1F600}", "\\x{1F600}$", "^.\\z", "a.a", ascii_only=False),
              f"a 4-byte character with {k} bytes before the boundary")
    # the match exists only through $ / only through (?m)^ right after a newline that ends a tile
    check(hx, [fill(T_ - 1) + b"\n" + b"b", fill(T_ - 1) + b"\n", fill(T_ - 2) + b"\nab", fill(2 * T_ - 1) + b"\n" + b"b" + fill(9)],
          rx("(?m)^b", "(?m)a$", "a$", "\\n$", "(?m)^$", "(?m)^ab$"), "look-ahead across the tile boundary")


def test_dfa_shapes_and_both_table_paths(handle):
    spec, a, hx, T_ = handle
    rng = np.random.default_rng(5)
    strings = [rng.integers(0, 256, int(n)).astype(np.uint8).tobytes() for n in rng.integers(0, 40, 2 * BLOCK + 9)]
    strings[7] = rng.integers(0, 256, T_ + 77).astype(np.uint8).tobytes()
    everything, nothing = R.compile_regex("", True), R.compile_regex("[^\\x00-\\x{10FFFF}]", True)
    assert everything.n_states == 1 and nothing.n_states == 1 and nothing.flags[0] == R.DEAD
    got, rep = check(hx, strings, [everything, nothing], "one state")
    assert int(np.unpackbits(got[0].view(np.uint8)).sum()) == len(strings) and not got[1].any()
    wide = random_table(12, 256, 1)                                  # 256 classes, 6 KiB: the LDS path
    big = random_table(300, 256, 2, absorbing=False)                 # 150 KiB: the global path
    assert wide.n_classes == 256 and big.table.nbytes > 96 * 1024
    _, rep = check(hx, strings, [wide], "256 classes")
    assert (rep["n_lds"], rep["n_global"]) == (1, 0) and wide.table.nbytes <= rep["table_lds_bytes"]
    _, rep = check(hx, strings, [big], "a table larger than the LDS budget")
    assert (rep["n_lds"], rep["n_global"]) == (0, 1)
    # the same tables forced down the other path give identical bits
    pats = [wide] + rx("ab|\\xff", "(a|b)*a(a|b){9}", ascii_only=False)
    lds, rep = check(hx, strings, pats, "LDS")
    assert rep["n_lds"] == len(pats)
    hx.tune("match_lds", 0)
    try:
        glb, rep = check(hx, strings, pats, "global")
        assert rep["n_global"] == len(pats) and rep["table_lds_bytes"] == 0
    finally:
        hx.tune("match_lds", 32)
    assert np.array_equal(lds, glb)
    # several DFAs in one call (both paths in one call) equal each DFA alone
    batch = [wide, big, everything, nothing] + rx("a", "\\x00")
    together, rep = check(hx, strings, batch, "batch")
    assert rep["n_lds"] == 5 and rep["n_global"] == 1
    for j, d in enumerate(batch):
        alone, _ = check(hx, strings, [d])
        assert np.array_equal(alone[0], together[j])


def test_small_workspace_runs_in_chunks_with_the_same_bits(handle):
    """805 strings are 4 blocks of 32 bytes of verdict words per DFA.  5 900 bytes hold the three small images (512 each), the 4 096 fixed
    bytes and two blocks per DFA: chunks of 512 strings.  170 kB hold one 150 KiB image but not two: one DFA at a time.  The bits
    must not depend on it, and a budget that holds no chunk is an error, not a failed launch."""
    spec, a, _, T_ = handle
    strings = short_strings(3 * BLOCK + 37, 3)
    small = rx("ab", "(?m)^a", "b$")
    big = [random_table(300, 256, 2, absorbing=False), random_table(290, 256, 3)]
    for budget, dfas, groups in ((5_900, small, 1), (170_000, big, 2), (1 << 26, small + big, 1)):
        hx = hip_index(a, workspace_bytes=budget)
        try:
            hx.set_columns({"s": ["x"] * N_DOCS})
            _, rep = check(hx, strings, dfas, f"budget {budget}")
            assert rep["n_chunks"] >= groups and (rep["n_chunks"] > 1) == (budget < (1 << 26)), (budget, rep)
        finally:
            hx.close()
    tight = hip_index(a, workspace_bytes=4_000)
    try:
        tight.set_columns({"s": ["x"] * N_DOCS})
        tight.set_column_text_raw(0, strings)
        with pytest.raises(MemoryError, match="workspace budget"):       # NP_ERR_OUT_OF_MEMORY
            tight.text_match_raw(0, [small[0].pack()], len(strings))
        w = small[0].pack()
        with pytest.raises(MemoryError, match="workspace budget"):
            tight.filter_ids([npa.filters.CompiledFilter([(npa.filters.NP_F_MATCH, 0, 0, w.size, 0)], w.astype(np.int64))])
    finally:
        tight.close()


# ---- through the filter -----------------------------------------------------------------------------------------------------

CONDS = [("t REGEXP ?", ["^al"]), ("t NOT REGEXP ?", ["a$"]), ("t LIKE ?", ["%a%"]), ("NOT (t LIKE ?)", ["be%"]),
         ("s REGEXP ? AND y > ?", ["(?i)^ab", 0]), ("s NOT REGEXP ? OR z = ?", ["b", 1]), ("t REGEXP ? AND t LIKE ? AND z < ?", ["é|z9", "%_", 3]),
         ("NOT (s REGEXP ? OR t REGEXP ?)", ["c$", "^[A-D]"]), ("s REGEXP ?", [None]), ("s LIKE ? OR w > ?", ["a_c", 0.5]),
         ("t REGEXP ?", ["(?m)^$"]), ("s IS NULL OR s REGEXP ?", [""])]


@pytest.fixture(scope="module")
def filtered(handle):
    spec, a, _, _ = handle
    rows = FR.make_rows(N_DOCS, seed=8)
    hx = hip_index(a)
    hx.set_columns(rows, text_on_device=["s", "t"])
    sch = hx.schema
    progs = [npa.compile_filter(c, p, sch) for c, p in CONDS]
    want = [RR.select(p, sch) for p in progs]
    yield spec, a, hx, rows, progs, want
    hx.close()


def test_filter_ids_equal_the_restated_ids(filtered):
    spec, a, hx, rows, progs, want = filtered
    assert sum(o[0] == npa.filters.NP_F_MATCH for p in progs for o in p.ops) >= 12
    got = hx.filter_ids(progs)
    for (cond, _), g, w in zip(CONDS, got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), cond
    assert want[8].size == 0 and 0 < want[0].size < N_DOCS and 0 < want[1].size < N_DOCS
    nulls = np.flatnonzero(np.ma.getmaskarray(rows["t"]))
    assert nulls.size and not np.isin(nulls, want[0]).any() and not np.isin(nulls, want[1]).any()   # UNKNOWN under NOT too
    assert [g.tolist() for g in hx.filter_ids(CONDS)] == [w.tolist() for w in want]               # compiled by the handle


def test_searches_with_filters_equal_subsets_of_the_ids(filtered):
    spec, a, hx, rows, progs, want = filtered
    pick = [0, 1, 4, 5, 8, 2]
    qs = list(synth.make_queries(spec, len(pick), n_tokens=6, cen=a["centroids"])[0])
    fl, subs = [CONDS[i] for i in pick], [want[i] for i in pick]
    p = npa.SearchParameters(n_full_scores=64, top_k=8, n_ivf_probe=4)
    same = lambda x, y: all(np.array_equal(r.passage_ids, s.passage_ids) and r.scores.tobytes() == s.scores.tobytes() for r, s in zip(x, y))
    assert same(hx.search_batch(qs, p, filters=fl), hx.search_batch(qs, p, subsets=subs))
    assert same(hx.search_exact(qs, 8, 0, filters=fl), hx.search_exact(qs, 8, 0, subsets=subs))
    assert hx.search_batch(qs, p, filters=fl)[4].passage_ids.size == 0 and hx.search_batch(qs, p, filters=fl)[0].passage_ids.size > 0
    data = T.TextIndexData.from_texts(TR.make_texts(N_DOCS, 10, seed=4, every="wo0", lens=(1, 2, 3, 5)))
    hx.set_text(data)
    try:
        tq = [T.TextQuery.from_phrases([[data.vocab["wo0"]]], T.NP_TEXT_AND)] * 3
        x = hx.text_search(tq, 10, filters=fl[:3])
        assert same(x, hx.text_search(tq, 10, subsets=subs[:3])) and x[0].passage_ids.size > 0
    finally:
        hx.set_text(None)


def test_two_shards_concatenate_to_the_whole(filtered):
    spec, a, hx, rows, progs, want = filtered
    parts = []
    for r in range(2):
        sh = hip_index(a, shard_rank=r, shard_count=2)
        try:
            sh.set_columns(rows, text_on_device=["s", "t"])              # the whole dictionary on every rank: codes are global
            parts.append(sh.filter_ids(progs))
        finally:
            sh.close()
    for j, w in enumerate(want):
        assert np.array_equal(np.concatenate([parts[0][j], parts[1][j]]), w), CONDS[j][0]
    assert all(len(parts[r][0]) > 0 for r in range(2))


def test_errors_leave_the_handle_usable(filtered):
    spec, a, hx, rows, progs, want = filtered
    F = npa.filters
    before = hx.info.device_bytes
    other = hip_index(a)
    try:
        other.set_columns(rows)                                          # no text on the device
        bare = other.info.device_bytes
        with pytest.raises(ValueError, match="no text"):
            other.filter_ids([progs[0]])
        with pytest.raises(ValueError, match="no text"):
            other.text_match_raw(4, [R.compile_regex("a", True).pack()], 10)
        with pytest.raises(ValueError, match="not a CODE column"):
            other.set_column_text_raw(0, [b"a"])                         # column 0 is y
        n_t = len(other.schema["t"].dictionary)
        with pytest.raises(ValueError, match="do not cover"):
            other.set_column_text_raw(5, [b"a"] * (n_t - 1))             # too few strings for the codes
        assert other.info.device_bytes == bare
        other.set_column_text_raw(5, other.schema["t"].dictionary)
        assert other.info.device_bytes > bare
        assert np.array_equal(other.filter_ids([progs[0]])[0], want[0])
        with pytest.raises(ValueError, match="string 1 has .* bytes, at most"):      # one lane walks one string: bounded
            other.set_column_text_raw(5, [b"a"] * 1 + [b"a" * (256 * tile_bytes(hx) + 1)] + [b"a"] * (n_t - 2))
        assert np.array_equal(other.filter_ids([progs[0]])[0], want[0])              # the previous text stays in place
        other.set_columns(rows)                                          # drops the text with the columns
        assert other.info.device_bytes == bare
        with pytest.raises(ValueError, match="no text"):
            other.filter_ids([progs[0]])
    finally:
        other.close()
    # a corrupt table: one transition past the last state, refused before any launch, naming the state
    good = R.compile_regex("ab+c", True)
    bad = R.Dfa(good.start, good.class_of, good.table.copy(), good.flags)
    bad.table[2, 1] = good.n_states
    with pytest.raises(ValueError, match="DFA 1, state 2"):
        hx.text_match_raw(5, [good.pack(), bad.pack()], len(hx.schema["t"].dictionary))
    prog = F.CompiledFilter([(F.NP_F_MATCH, 5, 0, bad.pack().size, 0)], bad.pack().astype(np.int64))
    with pytest.raises(ValueError, match="filter 0, op 0.*state 2"):
        hx.filter_ids([prog])
    short = F.CompiledFilter([(F.NP_F_MATCH, 5, 0, 10, 0)], good.pack().astype(np.int64))
    with pytest.raises(ValueError, match="op 0"):
        hx.filter_ids([short])
    with pytest.raises(ValueError, match="CODE column"):
        hx.filter_ids([F.CompiledFilter([(F.NP_F_MATCH, 0, 0, good.pack().size, 0)], good.pack().astype(np.int64))])
    assert hx.info.device_bytes == before
    assert np.array_equal(hx.filter_ids([progs[0]])[0], want[0])
    assert [m.tolist() for m in hx.match_text("t", ["^al", "a$"])] == \
        [[bool(__import__("re").search(p, s.decode())) for s in hx.schema["t"].dictionary] for p in ("^al", "a\\Z")]
    assert hx.match_text("s", ["A_C"], like=True)[0].tolist() == [s.decode().lower() in ("abc", "a_c", "a%c") for s in hx.schema["s"].dictionary]


def test_two_threads_on_one_handle(filtered):
    spec, a, hx, rows, progs, want = filtered
    serial = [g.tobytes() for g in hx.filter_ids(progs)]
    assert serial == [w.tobytes() for w in want]
    out, errs = {}, []

    def work(k):
        try:
            for r in range(4):
                mine = progs[k::2] if r % 2 == 0 else progs
                out[(k, r)] = ([g.tobytes() for g in hx.filter_ids(mine)], serial[k::2] if r % 2 == 0 else serial)
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, errs
    assert len(out) == 8 and all(got == exp for got, exp in out.values())


def test_cpp_mirror_gives_the_same_bits(filtered, tmp_path):
    spec, a, hx, rows, progs, want = filtered
    exe = tmp_path / "text_match"
    lib_dir = os.path.dirname(npa.library_path())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "text_match.cpp"),
                           "-I", os.path.join(ROOT, "next-plaid_amd", "cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib_dir, "-lnextplaid_hip", f"-Wl,-rpath,{lib_dir}"])
    ixdir = tmp_path / "ix"
    ixdir.mkdir()
    synth.write_index(str(ixdir), {k: v for k, v in a.items() if k != "_prep"}, chunk_docs=400)
    col = hx.schema["t"]
    text, off = col.text_arrays()
    files = {"codes.i32": col.data.astype("<i4"), "valid.u8": (col.valid if col.valid is not None else np.ones(N_DOCS, np.uint8)),
             "z.i64": np.asarray(rows["z"]).astype("<i8"), "text.bytes": text, "off.i64": off.astype("<i8"),
             "d0.u32": R.compile_regex("a$|^Do", False).pack().astype("<u4"), "d1.u32": R.compile_like("%é%").pack().astype("<u4")}
    for name, arr in files.items():
        np.ascontiguousarray(arr).tofile(tmp_path / name)
    out = subprocess.check_output([str(exe), str(ixdir)] + [str(tmp_path / n) for n in files], text=True, timeout=120)
    sch = npa.make_schema({"t": rows["t"], "z": rows["z"]}, N_DOCS, text_on_device=["t"])
    m = hx.match_text("t", [R.Dfa.unpack(files["d0.u32"]), R.Dfa.unpack(files["d1.u32"])])
    exp = "".join(f"match {j} " + "".join("1" if b else "0" for b in row) + "\n" for j, row in enumerate(m))
    conds = [("t REGEXP ?", ["a$|^Do"]), ("NOT (t LIKE ?)", ["%é%"]), ("t REGEXP ? AND z < ?", ["a$|^Do", 2]), ("t REGEXP ? OR t LIKE ?", ["a$|^Do", "%é%"])]
    for j, (c, p) in enumerate(conds):
        ids = RR.select(npa.compile_filter(c, p, sch), sch)
        exp += f"ids {j} {ids.size}" + "".join(f" {i}" for i in ids.tolist()) + "\n"
    assert out == exp and m[0].any() and m[1].any()
