#!/usr/bin/env python3
"""Time MmapIndex.update_resident (np_hip_index_expand) beside MmapIndex.update (directory update + reload) on synthetic index
directories, and write profiles/expand_time.md.

For each corpus size (documents x 300 tokens, K = 2^16, dim 128, 4 bits, written as tools/append_time.py writes them) the
directory is written once and copied: directory A is driven by update() (the directory update, then reload()), directory B by
update_resident() on a handle that stays open.  Both receive the same batches in the same order, so at every step they hold
the same index.  A batch is 300 / 3 000 / 30 000 new documents whose tokens are random unit vectors -- far from every
centroid, so the update clusters them into NEW centroids -- preceded by an untimed update of 50 such documents that stay in the
buffer, so that the timed call replaces a tail (n_reindexed = 50).  Per batch size and round the two are timed one after the
other, their order alternating; update_resident runs in odd rounds after reserve() and in even rounds without.  Every call is
one row of the table, with K before and after: the first expansion of a K = 65 536 index is the one that widens the codes.
NP_APPEND_TRACE=1 makes the library print the stages of the expand (tag "np expand"), captured per call.

With --parent-lib (the library built from the parent commit) the plain np_hip_index_append, which shares code with the new
entry, is timed against it: --parent-rounds rounds alternating the parent's library and this tree's (and which goes first),
each in its own process on the same seeded index; the allowed difference is the spread of the parent's own rounds.  Needs an
MI355X; there is no fallback.

    python tools/expand_time.py --out profiles/expand_time.md [--sizes 100000 1000000] [--rounds 2] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "next-plaid_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["NP_APPEND_TRACE"] = "1"

import numpy as np  # noqa: E402

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import api, synth  # noqa: E402
from append_time import CapturedStderr, write_directory  # noqa: E402

STAGES = ["grow", "centroids + bounds", "codes widened", "tail saved", "upload + token stages", "distinct-code rebuild",
          "posting-list cut + merge", "range table", "swap"]
LINE = re.compile(r"\[np expand\] (.+?)\s+([0-9.]+) s")
BUFFERED = 50


def far_docs(rng, n, doc_len, dim):
    x = rng.standard_normal((n * doc_len, dim)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return [x[i * doc_len:(i + 1) * doc_len] for i in range(n)]


def ms(t):
    return f"{t * 1e3:.1f}"


def measure(n_docs, args, work, lines):
    a_dir, b_dir = os.path.join(work, f"a_{n_docs}"), os.path.join(work, f"b_{n_docs}")
    t0 = time.perf_counter()
    write_directory(a_dir, n_docs, args.doc_len, args.centroids, args.dim, args.nbits, seed=1236)
    shutil.copytree(a_dir, b_dir)
    lines.append(f"\n## {n_docs:,} documents x {args.doc_len} tokens\n")
    lines.append(f"Directory written and copied in {time.perf_counter() - t0:.1f} s.\n")
    print(f"[expand_time] {n_docs} documents: directories written", flush=True)
    cfg = npa.UpdateConfig(start_from_scratch=-1)
    rng = np.random.default_rng(5)
    ha, hb = npa.MmapIndex.load(a_dir), npa.MmapIndex.load(b_dir)
    rows = []
    try:
        for r in range(args.rounds):
            for b in args.batches:
                print(f"[expand_time] {n_docs} documents: round {r}, {b} new", flush=True)
                buffered, docs = far_docs(rng, BUFFERED, args.doc_len, args.dim), far_docs(rng, b, args.doc_len, args.dim)
                ha.update(buffered, cfg)
                hb.update_resident(buffered, cfg)
                assert ha.last_update["mode"] == hb.last_update["mode"] == "buffer", (ha.last_update, hb.last_update)
                reserved = r % 2 == 1
                row = {"n": hb.num_documents(), "batch": b, "reserved": reserved, "k0": hb.num_partitions()}
                for who in ("ab" if (r + args.batches.index(b)) % 2 == 0 else "ba"):
                    if who == "a":
                        t0 = time.perf_counter()
                        _, rep = npa.update_index_dir(a_dir, docs, cfg)
                        t1 = time.perf_counter()
                        ha.reload()
                        t2 = time.perf_counter()
                        row.update(update_dir=t1 - t0, reload=t2 - t1, update=t2 - t0)
                    else:
                        if reserved:
                            hb.reserve(b + BUFFERED, (b + BUFFERED) * args.doc_len)
                        with CapturedStderr() as cap:
                            t0 = time.perf_counter()
                            hb.update_resident(docs, cfg)
                            row["resident"] = time.perf_counter() - t0
                        rep = hb.last_update
                        row["resident_dir"] = 1e-3 * (rep["ms_encode"] + rep["ms_outliers"] + rep["ms_kmeans"] + rep["ms_files"])
                        row["stages"] = {name.strip(): float(sec) for name, sec in LINE.findall(cap.text)}
                        row.update(mode=rep["mode"], k_new=rep["n_new_centroids"], n_reindexed=rep["n_reindexed"])
                row["k1"] = hb.num_partitions()
                assert ha.num_documents() == hb.num_documents() and ha.num_partitions() == hb.num_partitions()
                rows.append(row)
    finally:
        ha.close()
        hb.close()
    shutil.rmtree(a_dir, ignore_errors=True)
    shutil.rmtree(b_dir, ignore_errors=True)
    lines.append("Milliseconds of the host clock; one row per call.  `update()` = the directory update + `reload()`; "
                 "`update_resident()` = the same directory update + reading back what it wrote + `np_hip_index_expand`, whose own "
                 "stages (each ends in a device synchronise) follow.  `directory` is the library's report of its own work on the "
                 "directory (encode, outliers, k-means, files), which both calls pay.\n")
    head = ["documents", "new", "reserve", "K before -> after", "codes widened", "replaced", "update()", "of which reload()", "update_resident()",
            "directory", "expand stages together", "reload() / expand", "update() / update_resident()"] + STAGES
    lines.append("| " + " | ".join(head) + " |")
    lines.append("|" + "---|" * len(head))
    for w in rows:
        st = w["stages"]
        tot = sum(st.values())
        lines.append("| " + " | ".join(
            [f"{w['n']:,}", f"{w['batch']:,}", "yes" if w["reserved"] else "no", f"{w['k0']} -> {w['k1']}",
             "yes" if w["k0"] <= 65536 < w["k1"] else "no", str(w["n_reindexed"]), ms(w["update"]), ms(w["reload"]), ms(w["resident"]),
             ms(w["resident_dir"]), ms(tot), f"{w['reload'] / tot:.1f}x" if tot > 0 else "-", f"{w['update'] / w['resident']:.2f}x"] +
            [ms(st[s]) if s in st else "-" for s in STAGES]) + " |")
    slower = [w for w in rows if w["resident"] >= w["update"]]
    lines.append("")
    lines.append("`update_resident()` beat `update()` in every call." if not slower else
                 "`update_resident()` did NOT beat `update()` at: " + ", ".join(f"{w['n']:,} + {w['batch']:,}" for w in slower) + ".")
    return rows


def append_child(args):
    """the plain append_arrays through the library at --lib, bound by hand (the parent's library lacks the new entries).  Prints
    one JSON line: per count the median milliseconds of the round's calls"""
    api._preload_hip_runtime()
    L = C.CDLL(args.lib)
    vp, i64 = C.c_void_p, C.c_int64
    L.np_hip_last_error.restype = C.c_char_p
    L.np_hip_index_synth.argtypes = [C.POINTER(api.np_synth_spec), C.POINTER(api.np_open_opts), C.POINTER(vp)]
    L.np_hip_index_info.argtypes = [vp, C.POINTER(api.np_info)]
    L.np_hip_index_export.argtypes = [vp] * 6
    L.np_hip_index_ivf_size.argtypes = [vp]
    L.np_hip_index_ivf_size.restype = i64
    L.np_hip_index_reserve.argtypes = [vp, i64, i64]
    L.np_hip_index_append.argtypes = [vp, vp, i64, vp, vp]
    L.np_hip_index_remove.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.np_hip_index_close.argtypes = [vp]
    L.np_hip_index_close.restype = None
    api._lib = L   # MmapIndex's synth / reserve / remove_ids / append_arrays reach exactly these
    n = args.sizes[0]
    spec = synth.SynthSpec(num_docs=n, num_centroids=args.centroids, dim=args.dim, nbits=args.nbits, doc_len_min=args.doc_len,
                           doc_len_max=args.doc_len, seed=1236)
    big = synth.SynthSpec(num_docs=n + max(args.batches), num_centroids=args.centroids, dim=args.dim, nbits=args.nbits,
                          doc_len_min=args.doc_len, doc_len_max=args.doc_len, seed=1236)
    hx = npa.MmapIndex.synth(spec)
    out = {"lib": args.lib}
    try:
        hx.reserve(max(args.batches), max(args.batches) * args.doc_len)
        for b in args.batches:
            codes, res, lens = synth.doc_tokens(big, n, n + b)
            t = []
            for r in range(args.child_calls + 1):   # the first one is the warm-up
                t0 = time.perf_counter()
                hx.append_arrays(lens, codes, res)
                t1 = time.perf_counter()
                hx.remove_ids(np.arange(n, n + b))   # back to the index as it was (the capacity stays)
                if r:
                    t.append(1e3 * (t1 - t0))
            out[str(b)] = round(statistics.median(t), 3)
    finally:
        hx.close()
    print(json.dumps(out), flush=True)


def append_against_parent(args, lines):
    libs = {"p": os.path.abspath(args.parent_lib), "t": os.path.abspath(api.library_path())}
    rounds = []
    for i in range(args.parent_rounds):
        got = {}
        for who in ("pt" if i % 2 == 0 else "tp"):   # which of the two goes first alternates too
            cmd = [sys.executable, os.path.abspath(__file__), "--one=append", f"--lib={libs[who]}", "--sizes", str(args.parent_docs),
                   "--batches"] + [str(b) for b in args.batches] + \
                  [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("child_calls", "doc_len", "centroids", "dim", "nbits")]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
            if p.returncode != 0:   # a device error above all: nothing more is started on that GPU
                raise SystemExit(f"--one=append with {libs[who]}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
            got[who] = json.loads([x for x in p.stdout.strip().splitlines() if x.startswith("{")][-1])
        rounds.append((got["p"], got["t"]))
        print(json.dumps({"round": len(rounds), "parent": got["p"], "tree": got["t"]}), flush=True)
    lines.append("\n## np_hip_index_append against the parent commit's library\n")
    lines.append(f"`np_hip_index_append` shares its stages with the new entry.  One seeded index of {args.parent_docs:,} documents x "
                 f"{args.doc_len} tokens generated in HBM, {len(rounds)} rounds alternating the parent's library and this tree's (and which "
                 f"goes first), every round in its own process; a round's figure is the median of {args.child_calls} `append_arrays` calls "
                 "(with a reservation; the appended documents are removed again, untimed) after one warm-up, in milliseconds.  The allowed "
                 "difference is the spread of the parent's own rounds.\n")
    lines.append("| new documents | parent: rounds | this tree: rounds | parent median | parent spread | this tree median | difference | inside the parent's spread |")
    lines.append("|---|---|---|---|---|---|---|---|")
    for b in args.batches:
        ps, ts = [p[str(b)] for p, _ in rounds], [t[str(b)] for _, t in rounds]
        mp, mt, sp = statistics.median(ps), statistics.median(ts), max(ps) - min(ps)
        lines.append(f"| {b:,} | {' '.join(f'{x:.2f}' for x in ps)} | {' '.join(f'{x:.2f}' for x in ts)} | {mp:.2f} | {sp:.2f} | {mt:.2f} | "
                     f"{mt - mp:+.2f} | {'yes' if mt - mp <= sp else 'NO'} |")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_time.md"))
    ap.add_argument("--sizes", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--batches", type=int, nargs="+", default=[300, 3000, 30000])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--work", default=None, help="directory for the synthetic index directories (default: a temporary one)")
    ap.add_argument("--parent-lib", default="", help="libnextplaid_hip.so built from the parent commit: times np_hip_index_append against it")
    ap.add_argument("--parent-rounds", type=int, default=4)
    ap.add_argument("--parent-docs", type=int, default=1_000_000)
    ap.add_argument("--child-calls", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one child process may take")
    ap.add_argument("--one", choices=["append"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one == "append":
        return append_child(args)
    if npa.device_count() < 1:
        raise SystemExit("expand_time.py needs a gfx950 GPU: a time is a GPU measurement or it is not one")
    work = args.work or tempfile.mkdtemp(prefix="np_expand_")
    os.makedirs(work, exist_ok=True)
    lines = ["# Expanding a resident index against updating and reloading it", "",
             f"`python tools/expand_time.py --sizes {' '.join(map(str, args.sizes))} --rounds {args.rounds}` on one MI355X: K = "
             f"{args.centroids} at the start, dim {args.dim}, {args.nbits} bits, documents of {args.doc_len} tokens; the new documents' "
             "tokens are random unit vectors, so every update adds centroids.  No ratio is fixed in advance: the table records what "
             "was measured."]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    for n in args.sizes:
        try:
            measure(n, args, work, lines)
        except (MemoryError, OSError) as e:   # a size that does not fit this machine's memory or disk: say so, keep what was
            # measured.  Anything else -- a device error above all -- ends the run: nothing more is started on that GPU
            lines.append(f"\n## {n:,} documents: NOT MEASURED ({type(e).__name__}: {e})\n")
        save()
    if args.parent_lib:
        append_against_parent(args, lines)
        save()
    if not args.work:
        shutil.rmtree(work, ignore_errors=True)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
