#!/usr/bin/env python3
"""Times np_hip_text_match on the device beside the two host ways to answer the same question.

  timeout 900 python tools/match_time.py          # writes profiles/match_time.md and prints one JSON line per measurement

Two seeded synthetic dictionaries, generated here (nothing is read from anywhere):
    paths   --paths strings like "src/index/mod_17/search_batch.rs": tens of bytes
    code    --code strings of about 1 KB: 20 lines drawn from a pool of identifier / operator lines
Three patterns per dictionary:
    small   a REGEXP whose table fits the LDS budget, timed down BOTH table paths (np_hip_index_tune "match_lds")
    large   a REGEXP whose table exceeds the budget (a bounded gap, x.{8}y: about 2 k states x 14 byte classes, 64 KB), global path
    like    LIKE '%x%' with a literal x that occurs in some strings
Per (dictionary, pattern), wall-clock per call from Python (every device call ends in a synchronise inside the library and
includes the upload of the table and the read-back of the bits).  A sample is a loop of calls that fills 50 ms; the table gives
the median, the minimum and the maximum of --repeats samples after --warmup untimed calls: a difference inside that spread is none:
    device      MmapIndex.text_match_raw, one DFA over the whole dictionary
    host re     the loop _Compiler.like runs today: a compiled Python `re` over every dictionary string (search for REGEXP,
                fullmatch for LIKE), once (it is seconds long)
    sqlite      SELECT count(*) FROM t WHERE s LIKE ? over the same strings in an in-memory table (LIKE rows only), once
GB/s = dictionary bytes / device time: an end-to-end rate of the call, not a kernel's share of peak.  The device's verdicts are
compared with the host loop's on every string.  No ratio is asserted anywhere; the table is what was measured, and where the
device does not beat the host loop it replaces, the row says so.  Run it under a time limit, as above: every step that touches
the GPU is one bounded call, and the tool stops at the first error.
"""
import argparse
import json
import os
import re
import sqlite3
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import regexes as R, synth  # noqa: E402


def make_paths(n, seed):
    rng = np.random.default_rng(seed)
    dirs = ["src", "lib", "tests", "index", "search", "filter", "codec", "api", "tools", "docs", "bench", "kernels", "text", "util"]
    stems = ["mod", "search_batch", "filter_eval", "kmeans", "update", "loader", "writer", "plan", "match", "regexp", "fusion", "pool"]
    exts = [".rs", ".py", ".hip", ".h", ".cpp", ".md", ".toml"]
    d = rng.integers(0, len(dirs), (n, 3))
    k = rng.integers(1, 4, n)
    s = rng.integers(0, len(stems), n)
    e = rng.integers(0, len(exts), n)
    num = rng.integers(0, 1000, n)
    return [("/".join(dirs[j] for j in d[i, :k[i]]) + f"/{stems[s[i]]}_{num[i]}{exts[e[i]]}").encode() for i in range(n)]


def make_code(n, seed, lines_per=20):
    rng = np.random.default_rng(seed)
    words = ["let", "fn", "return", "index", "search", "query", "score", "top_k", "for", "in", "if", "else", "self", "vec", "len", "push",
             "filter", "regexp", "match", "code", "unit", "doc", "ids", "subset", "yield", "x", "y", "n"]
    ops = [" = ", "(", ")", ", ", " + ", ".", "::", " -> ", " {", "}", ";", " < ", "[", "]", " // "]
    pool = []
    for _ in range(4096):
        k = int(rng.integers(5, 12))
        pool.append(("    " * int(rng.integers(0, 3)) + "".join(words[int(rng.integers(0, len(words)))] + ops[int(rng.integers(0, len(ops)))]
                                                              for _ in range(k)) + "\n").encode())
    idx = rng.integers(0, len(pool), (n, lines_per))
    return [b"".join(pool[j] for j in row) for row in idx]


def timed_ms(fn, repeats, warmup, window_s=0.05):
    """(min, median, max) ms per call over `repeats` samples.  A sample is a loop of as many calls as fill window_s (counted
    from one untimed call), so that a 0.1 ms call is not timed against the clock's and the scheduler's noise."""
    for _ in range(warmup):
        fn()
    t0 = time.perf_counter()
    fn()
    loops = max(1, int(window_s / max(time.perf_counter() - t0, 1e-6)))
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(loops):
            fn()
        ts.append(1e3 * (time.perf_counter() - t0) / loops)
    ts.sort()
    return ts[0], ts[len(ts) // 2], ts[-1], loops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1_000_000)
    ap.add_argument("--code", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_time.md"))
    args = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("match_time.py needs a gfx950 GPU: there is nothing to time without one")

    spec = synth.SynthSpec(num_docs=256, num_centroids=16, dim=32, nbits=2, doc_len_min=2, doc_len_max=4, seed=1)
    a = synth.generate_arrays(spec)
    hx = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"], a["codes"],
                                   a["residuals"], a["nbits"])
    hx.set_columns({"s": ["x"] * 256})      # every row holds code 0: any dictionary may be the column's text
    rows = []
    for name, strings, small, large, like in (("paths", make_paths(args.paths, 1), r"kernels/.*_7[0-9]*\.hip$", "s.{8}h", "%search_batch%"),
                                              ("code", make_code(args.code, 2), r"return\(regexp[.:]", "y.{8}q", "%yield::match%")):
        n_bytes = sum(len(s) for s in strings)
        texts = [s.decode() for s in strings]
        hx.set_column_text_raw(0, strings)
        con = sqlite3.connect(":memory:")
        con.execute("CREATE TABLE t (s TEXT)")
        con.executemany("INSERT INTO t VALUES (?)", ((t,) for t in texts))
        for kind, pattern in (("small", small), ("large", large), ("like", like)):
            dfa = R.compile_like(pattern) if kind == "like" else R.compile_regex(pattern, True)
            packed = dfa.pack()
            if kind == "like":
                rx = re.compile("".join(".*" if c == "%" else "." if c == "_" else re.escape(c) for c in pattern), re.DOTALL | re.IGNORECASE | re.ASCII)
                probe = rx.fullmatch
            else:
                rx = re.compile(pattern.replace("$", r"\Z"))
                probe = rx.search
            t0 = time.perf_counter()
            want = np.fromiter((probe(t) is not None for t in texts), bool, len(texts))
            host_ms = 1e3 * (time.perf_counter() - t0)
            sqlite_ms = None
            if kind == "like":
                t0 = time.perf_counter()
                n_sql = con.execute("SELECT count(*) FROM t WHERE s LIKE ?", [pattern]).fetchone()[0]
                sqlite_ms = 1e3 * (time.perf_counter() - t0)
                assert n_sql == int(want.sum()), (n_sql, int(want.sum()))
            for lds_kib in ((32, 0) if kind == "small" else (32,)):
                hx.tune("match_lds", lds_kib)
                bits = hx.text_match_raw(0, [packed], len(strings))
                rep = dict(hx.last_match_report)
                got = np.unpackbits(bits[0].view(np.uint8), bitorder="little")[:len(strings)].astype(bool)
                assert np.array_equal(got, want), f"{name} {kind}: the device and the host loop disagree on {int((got != want).sum())} strings"
                dev_min, dev_ms, dev_max, loops = timed_ms(lambda: hx.text_match_raw(0, [packed], len(strings)), args.repeats, args.warmup)
                row = {"dictionary": name, "strings": len(strings), "bytes": n_bytes, "pattern": pattern, "kind": kind,
                       "states": dfa.n_states, "classes": dfa.n_classes, "table_bytes": int(dfa.table.nbytes),
                       "path": "lds" if rep["n_lds"] else "global", "tile_bytes": rep["tile_bytes"], "matches": int(want.sum()),
                       "device_ms": round(dev_ms, 3), "device_ms_min": round(dev_min, 3), "device_ms_max": round(dev_max, 3),
                       "calls_per_sample": loops, "device_GBps": round(n_bytes / dev_ms / 1e6, 2), "host_re_ms": round(host_ms, 1),
                       "sqlite_like_ms": None if sqlite_ms is None else round(sqlite_ms, 1),
                       "device_beats_host_re": bool(dev_ms < host_ms)}
                print(json.dumps(row), flush=True)
                rows.append(row)
            hx.tune("match_lds", 32)
        con.close()
    hx.close()
    kept = ""                     # sections below the table that other measurements added by hand stay
    if os.path.exists(args.out):
        old = open(args.out).read()
        kept = old[old.index("\n## "):] if "\n## " in old else ""
    with open(args.out, "w") as f:
        f.write("# np_hip_text_match beside the host loop and SQLite's LIKE\n\n")
        f.write("Written by `tools/match_time.py` (its docstring says what each column is).  One DFA over the whole dictionary per call; "
                "device time is wall-clock around the call (table upload, kernel, read-back of the bits): median (min - max) of samples that "
                "loop the call for 50 ms each; GB/s is dictionary bytes over the median.  The host loop and SQLite ran once each.\n\n")
        f.write("| dictionary | strings | MB | pattern | states x classes | table path | matches | device ms: median (min - max) | calls per sample | GB/s | host re ms | SQLite LIKE ms | device beats the host loop |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            f.write(f"| {r['dictionary']} | {r['strings']} | {r['bytes'] / 1e6:.1f} | `{r['pattern']}` ({r['kind']}) | {r['states']} x {r['classes']} | "
                    f"{r['path']} | {r['matches']} | {r['device_ms']} ({r['device_ms_min']} - {r['device_ms_max']}) | {r['calls_per_sample']} | {r['device_GBps']} | {r['host_re_ms']} | "
                    f"{'-' if r['sqlite_like_ms'] is None else r['sqlite_like_ms']} | {'yes' if r['device_beats_host_re'] else 'NO'} |\n")
        f.write(kept)


if __name__ == "__main__":
    main()
