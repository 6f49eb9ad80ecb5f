#!/usr/bin/env python3
"""Times keeping the device keyword index current (np_hip_text_build_merge) beside the ways there were before.

  timeout 1700 python tools/textmerge_time.py [--parent-lib PATH]   # writes profiles/textmerge_time.md, one JSON line per measurement

Corpus: tools/textbuild_time.py's seeded one (--docs documents, default 300 000, unicode61) plus a tenth as many further
documents from the same generator to append and to replace with.  The base is TextIndexData.from_texts_device of the --docs
documents.  Operations: append 0.1 %, 1 % and 10 %; delete 1 % (seeded choice) with renumbering; replace 1 %.  Per operation,
in one child process:
    equal       the merge's arrays are compared with the whole-corpus rebuild's, array for array, before anything is timed
    merge       base.updated(...): `around` is wall-clock around the call (encoding, the batch's build, the checks, the merge,
                read-back, the Python list of terms), median (min - max) of --repeats calls after --warmup untimed ones;
                `library` is what the library reports for the median call: ms_total of the batch's np_hip_text_build plus
                ms_total of np_hip_text_build_merge; the merge's stages are beside it
    rebuild     TextIndexData.from_texts_device of the resulting rows, wall-clock, median of the same number of calls
                (np_hip_text_build: not the code under test)
    sqlite      the same operation on a live in-memory FTS5 table (a copy of the base table per operation; delete and insert
                statements; renumbering = drop the table and insert the survivors again, as rebuild does), once
    set_text    MmapIndex.set_text of the result on a handle of as many documents (what the host round trip still costs), once
With --parent-lib (the library built from the parent commit) np_hip_text_build is timed against it, because the scan launches
moved behind a header: --rounds rounds, alternating parent and this tree (and which of the two goes first), each call in its
own process; a round's figure is the median of --repeats calls after --warmup.  The allowed difference is the spread of the
parent's own rounds; both are written.
No ratio is asserted anywhere: the table is what was measured."""
import argparse
import ctypes as C
import json
import os
import sqlite3
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from textbuild_time import make_corpus   # noqa: E402

OPS = [("append 0.1 %", "append", 0.001), ("append 1 %", "append", 0.01), ("append 10 %", "append", 0.1),
       ("delete 1 % + renumber", "delete", 0.01), ("replace 1 %", "replace", 0.01)]


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def plan_op(kind, frac, n, extra):
    rng = np.random.default_rng(11)
    k = max(int(round(n * frac)), 1)
    if kind == "append":
        return dict(new_texts=extra[:k], delete=[], replace={})
    ids = sorted(int(i) for i in rng.choice(n, k, replace=False))
    if kind == "delete":
        return dict(new_texts=[], delete=ids, replace={})
    return dict(new_texts=[], delete=[], replace={d: extra[i] for i, d in enumerate(ids)})


def rows_after(texts, op):
    gone = set(op["delete"])
    rows = [op["replace"].get(i, t) for i, t in enumerate(texts) if i not in gone]
    return rows + list(op["new_texts"])


def ops_child(args):
    import next_plaid_amd as npa
    from next_plaid_amd import synth, text as T
    from next_plaid_amd.text import TextIndexData
    if npa.device_count() < 1:
        raise SystemExit("textmerge_time.py needs a gfx950 GPU: there is nothing to time without one")
    n = args.docs
    allt = make_corpus(n + n // 10, args.words, args.vocab, 7)
    texts, extra = allt[:n], allt[n:]
    base = TextIndexData.from_texts_device(texts)
    assert base.fallback_docs == []
    t0 = time.perf_counter()
    live = sqlite3.connect(":memory:")
    T.create_fts_tables(live, "unicode61", content_synced=False)
    T.insert_fts_rows(live, texts, range(n), "unicode61", content_synced=False)
    sqlite_build_s = time.perf_counter() - t0
    spec = synth.SynthSpec(num_docs=n + n // 10, num_centroids=64, dim=64, nbits=4, doc_len_min=1, doc_len_max=2, seed=9)
    a = synth.generate_arrays(spec)
    ix = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"], a["codes"],
                                   a["residuals"], a["nbits"], device=0)
    print(json.dumps({"base": {"docs": n, "instances": int(base.inst_doc.size), "terms": base.n_terms,
                               "sqlite_build_s": round(sqlite_build_s, 2)}}), flush=True)
    for label, kind, frac in OPS:
        op = plan_op(kind, frac, n, extra)
        kw = dict(delete=op["delete"], replace=op["replace"], renumber=True)
        rows = rows_after(texts, op)
        got = base.updated(op["new_texts"], **kw)
        want = TextIndexData.from_texts_device(rows)
        assert got.terms == want.terms and got.n_rows == want.n_rows == len(rows)
        for k in ("term_offsets", "inst_doc", "inst_pos"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), (label, k)
        merges, rebuilds = [], []
        for i in range(args.warmup + args.repeats):
            t0 = time.perf_counter()
            r = base.updated(op["new_texts"], **kw)
            t1 = time.perf_counter()
            TextIndexData.from_texts_device(rows)
            t2 = time.perf_counter()
            if i >= args.warmup:
                merges.append((1e3 * (t1 - t0), r.build_report))
                rebuilds.append(1e3 * (t2 - t1))
        merges.sort(key=lambda x: x[0])
        around, rep = merges[len(merges) // 2]
        batch = rep.get("batch") or {}
        # the live SQLite table: a copy of the base table, then the operation
        conn = sqlite3.connect(":memory:")
        live.backup(conn)
        t0 = time.perf_counter()
        with conn:
            for d in list(op["delete"]) + list(op["replace"]):
                conn.execute(f'DELETE FROM "{T.FTS_TABLE}" WHERE rowid = ?', (d,))
        T.insert_fts_rows(conn, list(op["replace"].values()), list(op["replace"]), "unicode61", content_synced=False)
        T.insert_fts_rows(conn, op["new_texts"], range(n, n + len(op["new_texts"])), "unicode61", content_synced=False)
        if op["delete"]:
            conn.execute(f'DROP TABLE "{T.FTS_TABLE}"')
            T.create_fts_tables(conn, "unicode61", content_synced=False)
            T.insert_fts_rows(conn, rows, range(len(rows)), "unicode61", content_synced=False)
        sqlite_s = time.perf_counter() - t0
        assert int(conn.execute(f'SELECT count(*) FROM "{T.FTS_TABLE}_docsize"').fetchone()[0]) == len(rows)
        conn.close()
        t0 = time.perf_counter()
        ix.set_text(got)
        set_text_s = time.perf_counter() - t0
        ix.set_text(None)
        row = {"op": label, "batch_docs": len(op["new_texts"]) + len(op["replace"]), "deleted": len(op["delete"]),
               "instances_out": int(got.inst_doc.size), "terms_out": got.n_terms,
               "around_ms": [round(x, 1) for x in (around, merges[0][0], merges[-1][0])],
               "library_ms": round(rep["ms_total"] + batch.get("ms_total", 0.0), 1), "batch_build_ms": round(batch.get("ms_total", 0.0), 1),
               "merge_ms": {k[3:]: round(rep[k], 1) for k in ("ms_check", "ms_upload", "ms_count", "ms_terms", "ms_place", "ms_total")},
               "rebuild_ms": [round(x, 1) for x in med(rebuilds)], "sqlite_s": round(sqlite_s, 2), "set_text_s": round(set_text_s, 2),
               "workspace_MB": round(rep["workspace_bytes"] / 1e6, 1)}
        print(json.dumps(row), flush=True)


def build_child(args):
    """np_hip_text_build of the corpus through the library at --lib, by hand: the parent's library lacks the new entry, so
    api.lib() (which binds every entry) cannot load it."""
    from next_plaid_amd import api
    api._preload_hip_runtime()
    L = C.CDLL(args.lib)
    texts = make_corpus(args.docs, args.words, args.vocab, 7)
    raws = [t.encode() for t in texts]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    raw = np.frombuffer(b"".join(raws), np.uint8)
    L.np_hip_text_build.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(api.np_text_build_opts), C.POINTER(C.c_void_p),
                                    C.POINTER(api.np_text_build_report)]
    L.np_hip_text_build_free.argtypes = [C.c_void_p]
    L.np_hip_text_build_free.restype = None
    ms, inst = [], 0
    for i in range(args.warmup + args.repeats):
        o, rep, h = api.np_text_build_opts(0), api.np_text_build_report(), C.c_void_p()
        t0 = time.perf_counter()
        rc = L.np_hip_text_build(0, raw.ctypes.data, off.ctypes.data, len(raws), C.byref(o), C.byref(h), C.byref(rep))
        dt = 1e3 * (time.perf_counter() - t0)
        if rc != 0:
            raise SystemExit(f"np_hip_text_build: rc {rc}")
        L.np_hip_text_build_free(h)
        inst = int(rep.n_instances)
        if i >= args.warmup:
            ms.append(dt)
    print(json.dumps({"lib": args.lib, "instances": inst, "ms": round(med(ms)[0], 2)}), flush=True)


def child(args, *extra):
    cmd = [sys.executable, os.path.abspath(__file__)] + list(extra) + [f"--{k}={getattr(args, k)}" for k in
                                                                      ("docs", "words", "vocab", "repeats", "warmup")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
    if p.returncode != 0:
        raise SystemExit(f"{extra}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
    return [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--words", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--parent-lib", default="", help="libnextplaid_hip.so built from the parent commit: times np_hip_text_build against it")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "textmerge_time.md"))
    ap.add_argument("--one", choices=["ops", "build"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one == "ops":
        return ops_child(args)
    if args.one == "build":
        return build_child(args)
    rows = child(args, "--one=ops")
    for r in rows:
        print(json.dumps(r), flush=True)
    rounds = []
    if args.parent_lib:
        from next_plaid_amd import api
        libs = {"p": os.path.abspath(args.parent_lib), "t": os.path.abspath(api.library_path())}
        for i in range(args.rounds):
            got = {}
            for who in ("pt" if i % 2 == 0 else "tp"):      # which of the two goes first alternates too
                got[who] = child(args, "--one=build", f"--lib={libs[who]}")[-1]
            p, t = got["p"], got["t"]
            assert p["instances"] == t["instances"]
            rounds.append((p["ms"], t["ms"]))
            print(json.dumps({"round": len(rounds), "parent_ms": p["ms"], "tree_ms": t["ms"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    base = rows[0]["base"]
    with open(args.out, "w") as f:
        f.write("# Keeping the device keyword index current: the merge beside a rebuild and beside SQLite\n\n")
        f.write("Written by `tools/textmerge_time.py` (its docstring says what each column is).  unicode61; the seeded corpus of "
                f"`tools/textbuild_time.py`: {base['docs']} documents, {base['instances']} instances, {base['terms']} terms.  Every "
                "result equalled the whole-corpus rebuild's arrays before anything was timed.  Merge and rebuild: median (min - max) of "
                f"{args.repeats} calls after {args.warmup} warm-up, wall-clock around `TextIndexData.updated` and "
                "`TextIndexData.from_texts_device`; library = the batch's `np_hip_text_build` plus `np_hip_text_build_merge`, as the "
                "library reports them for the median call.  SQLite: the operation on a live in-memory FTS5 table (building that table "
                f"took {base['sqlite_build_s']} s), once; renumbering drops the table and inserts the survivors again.  set_text: "
                "`MmapIndex.set_text` of the result, once.  All on one machine in one run.\n\n")
        f.write("| operation | batch documents | deleted | instances out | merge around ms | library ms | of it the batch's build | "
                "merge: check | upload | count | strings | place | rebuild ms | live SQLite s | set_text s | device MB |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows[1:]:
            m, a, b = r["merge_ms"], r["around_ms"], r["rebuild_ms"]
            f.write(f"| {r['op']} | {r['batch_docs']} | {r['deleted']} | {r['instances_out']} | {a[0]} ({a[1]} - {a[2]}) | {r['library_ms']} | "
                    f"{r['batch_build_ms']} | {m['check']} | {m['upload']} | {m['count']} | {m['terms']} | {m['place']} | "
                    f"{b[0]} ({b[1]} - {b[2]}) | {r['sqlite_s']} | {r['set_text_s']} | {r['workspace_MB']} |\n")
        if rounds:
            ps, ts = [p for p, _ in rounds], [t for _, t in rounds]
            f.write("\n## np_hip_text_build against the parent commit's library\n\n")
            f.write("The scan launches moved from `np_textbuild.hip` into `np_textbuild_dev.h`, which the merge shares; beyond that only "
                    f"the wording of three messages changed in the build.  The same corpus, {len(rounds)} rounds alternating the parent's library and this tree's (and which goes first), "
                    f"every call in its own process; a round's figure is the median of {args.repeats} calls after {args.warmup} warm-up, wall-clock "
                    "around `np_hip_text_build`.  The allowed difference is the spread of the parent's own rounds.\n\n")
            f.write("| round | parent ms | this tree ms |\n|---|---|---|\n")
            for i, (p, t) in enumerate(rounds):
                f.write(f"| {i + 1} | {p} | {t} |\n")
            f.write(f"\nParent: median {med(ps)[0]}, spread {round(max(ps) - min(ps), 2)} ({min(ps)} - {max(ps)}).  This tree: median "
                    f"{med(ts)[0]} ({min(ts)} - {max(ts)}); the medians differ by {round(med(ts)[0] - med(ps)[0], 2)} ms.\n")


if __name__ == "__main__":
    main()
