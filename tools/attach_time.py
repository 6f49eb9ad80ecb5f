#!/usr/bin/env python3
"""Time the keeping remove and append (np_hip_index_remove_keep, np_hip_index_append_rows) beside the dropping calls plus the
setters, and write profiles/attach_time.md.

One synthetic index (documents x DOC_LEN tokens, generated in HBM) carries 8 columns -- two I64 (one with NULLs), two F64 (one
with NULLs), two CODE (one with its dictionary text on the device), and two more I64 -- and groups.  For every count (300 /
3 000 / 30 000 random documents) and round, alternating:
  keeping   remove_ids(ids, keep_attachments=True), then append_arrays(the same documents' tokens, rows=...) -- which also
            restores the document count;
  dropping  remove_ids(ids) + set_columns + set_column_text + set_groups of host arrays ALREADY PREPARED (typed, coded,
            renumbered: the host's own work is not counted), then append_arrays + the same setters.
NP_REMOVE_TRACE=1 makes the library print the compaction kernels' own time (device events) and the bytes they move.

With --parent-lib (the library built from the parent commit) the PLAIN np_hip_index_remove and np_hip_index_append -- whose
path gained a wrapper and an argument -- are timed against it: --parent-rounds rounds, alternating the parent's library and
this tree's (and which of the two goes first), each in its own process on the same seeded index without attachments; a round's
figure is the median of its calls.  The allowed difference is the spread of the parent's own rounds; the table says whether
this tree's median lies inside it.  The parent's library lacks the new entries, so the child binds the few entries it needs by
hand.  Needs an MI355X; there is no fallback.

    python tools/attach_time.py --out profiles/attach_time.md [--docs 1000000] [--rounds 3] [--parent-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "next-plaid_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["NP_REMOVE_TRACE"] = "1"

import numpy as np  # noqa: E402

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import api, filters as F, synth  # noqa: E402

COPY_RATE = 6.29e12   # bytes/s of a float4 copy measured on the MI355X (the micro-architecture guide's HBM figure)
KERNEL = re.compile(r"\[np remove\] attach kernel\s+([0-9.]+) s\s+(\d+) bytes")


class CapturedStderr:
    """fd 2 into a file for the duration: the library's trace lines are written by C"""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("utf-8", "replace")
        self.tmp.close()


def spread(xs):
    return f"{statistics.median(xs) * 1e3:.1f} ({min(xs) * 1e3:.1f}-{max(xs) * 1e3:.1f})"


def make_columns(n, seed=3):
    rng = np.random.default_rng(seed)
    words = [f"w{j:04d}" for j in range(2000)]
    tags = [f"tag-{j:03d}" for j in range(300)]
    return {"a": rng.integers(0, 1 << 40, n), "b": np.ma.masked_array(rng.integers(0, 99, n), rng.random(n) < 0.1),
            "x": rng.standard_normal(n), "y": np.where(rng.random(n) < 0.1, np.nan, rng.standard_normal(n)),
            "w": np.array(words)[rng.integers(0, len(words), n)], "t": np.array(tags)[rng.integers(0, len(tags), n)],
            "c": rng.integers(-5, 5, n), "d": np.arange(n)}, rng.integers(0, max(1, n // 20), n).astype(np.int32)


def set_prepared(hx, sch, gids, n_groups):
    """set_columns + set_column_text + set_groups of arrays that are ready"""
    cols = (api.np_column * len(sch))()
    for c in sch.columns.values():
        cols[c.index] = api.np_column(c.type, 0, c.data.ctypes.data, None if c.valid is None else c.valid.ctypes.data)
    api._check(api.lib().np_hip_index_set_columns(hx._h, cols, len(sch)))
    for c in sch.columns.values():
        if c.text_on_device:
            hx.set_column_text_raw(c.index, c.dictionary)
    hx.schema = sch
    hx.set_groups(gids, n_groups=n_groups)


def tokens_of(a, ids):
    off = np.concatenate([[0], np.cumsum(a["doc_lengths"])])
    pick = np.concatenate([np.arange(off[d], off[d + 1]) for d in ids])
    return a["doc_lengths"][ids], a["codes"][pick], a["residuals"][pick]


def plain_child(args):
    """the plain remove_ids and append_arrays through the library at --lib, bound by hand: api.lib() binds every entry, and the
    parent's library lacks the new ones.  Prints one JSON line: per count the median milliseconds of the round's calls"""
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
    api._lib = L   # MmapIndex's synth / export / reserve / remove_ids / append_arrays reach exactly these
    spec = synth.SynthSpec(num_docs=args.docs, num_centroids=args.centroids, dim=args.dim, nbits=args.nbits, doc_len_min=args.doc_len,
                           doc_len_max=args.doc_len, seed=1236)
    hx = npa.MmapIndex.synth(spec)
    out = {"lib": args.lib}
    try:
        a = hx.export()
        hx.reserve(max(args.counts), max(args.counts) * args.doc_len)
        rng = np.random.default_rng(7)
        for c in args.counts:
            ids = np.sort(rng.choice(args.docs, c, replace=False)).astype(np.int64)
            new = tokens_of(a, ids)
            rem, app = [], []
            for r in range(args.rounds + 1):   # the first one is the warm-up
                t0 = time.perf_counter()
                hx.remove_ids(ids)
                t1 = time.perf_counter()
                hx.append_arrays(*new)
                t2 = time.perf_counter()
                if r:
                    rem.append(1e3 * (t1 - t0)), app.append(1e3 * (t2 - t1))
            out[str(c)] = {"remove": round(statistics.median(rem), 3), "append": round(statistics.median(app), 3)}
    finally:
        hx.close()
    print(json.dumps(out), flush=True)


def plain_against_parent(args, lines):
    libs = {"p": os.path.abspath(args.parent_lib), "t": os.path.abspath(api.library_path())}
    rounds = []
    for i in range(args.parent_rounds):
        got = {}
        for who in ("pt" if i % 2 == 0 else "tp"):   # which of the two goes first alternates too
            cmd = [sys.executable, os.path.abspath(__file__), "--one=plain", f"--lib={libs[who]}", "--counts"] + [str(c) for c in args.counts] + \
                  [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("docs", "rounds", "doc_len", "centroids", "dim", "nbits")]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
            if p.returncode != 0:   # a device error above all: nothing more is started on that GPU
                raise SystemExit(f"--one=plain with {libs[who]}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
            got[who] = json.loads([x for x in p.stdout.strip().splitlines() if x.startswith("{")][-1])
        rounds.append((got["p"], got["t"]))
        print(json.dumps({"round": len(rounds), "parent": got["p"], "tree": got["t"]}), flush=True)
    lines.append("\n## The plain entries against the parent commit's library\n")
    lines.append("`np_hip_index_remove` and `np_hip_index_append` still drop the attachments; their path gained the entries' shared "
                 f"wrappers and one argument.  The same seeded index without attachments, {len(rounds)} rounds alternating the parent's "
                 f"library and this tree's (and which goes first), every round in its own process; a round's figure is the median of "
                 f"{args.rounds} calls after one warm-up, milliseconds around `remove_ids` / `append_arrays` (with a reservation).  The "
                 "allowed difference is the spread of the parent's own rounds.\n")
    lines.append("| documents | entry | parent: rounds | this tree: rounds | parent median | parent spread | this tree median | difference | inside the parent's spread |")
    lines.append("|---|---|---|---|---|---|---|---|---|")
    inside_all = True
    for c in args.counts:
        for entry in ("remove", "append"):
            ps, ts = [p[str(c)][entry] for p, _ in rounds], [t[str(c)][entry] for _, t in rounds]
            mp, mt, sp = statistics.median(ps), statistics.median(ts), max(ps) - min(ps)
            inside = mt - mp <= sp   # slower by no more than the parent differs from itself
            inside_all = inside_all and inside
            lines.append(f"| {c:,} | {entry} | {' '.join(f'{x:.2f}' for x in ps)} | {' '.join(f'{x:.2f}' for x in ts)} | {mp:.2f} | {sp:.2f} | "
                         f"{mt:.2f} | {mt - mp:+.2f} | {'yes' if inside else 'NO'} |")
    lines.append(f"\nEvery median inside the parent's own spread: {'yes' if inside_all else 'NO'}.")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attach_time.md"))
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--counts", type=int, nargs="+", default=[300, 3000, 30000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--doc-len", type=int, default=32)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--parent-lib", default="", help="libnextplaid_hip.so built from the parent commit: times the plain remove and append against it")
    ap.add_argument("--parent-rounds", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds one child process may take")
    ap.add_argument("--one", choices=["plain"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one == "plain":
        return plain_child(args)
    if npa.device_count() < 1:
        raise SystemExit("attach_time.py needs a gfx950 GPU: a time is a GPU measurement or it is not one")
    n = args.docs
    spec = synth.SynthSpec(num_docs=n, num_centroids=args.centroids, dim=args.dim, nbits=args.nbits, doc_len_min=args.doc_len,
                           doc_len_max=args.doc_len, seed=1236)
    values, gids = make_columns(n)
    n_groups = int(gids.max()) + 1
    sch = F.make_schema(values, n, text_on_device=["t"])
    lines = ["# Keeping columns and groups through a resident remove and append", "",
             f"`python tools/attach_time.py --docs {n} --rounds {args.rounds}` on one MI355X: {n:,} documents of {args.doc_len} tokens, "
             f"K = {args.centroids}, dim {args.dim}, {args.nbits} bits; 8 columns (I64, I64 with NULLs, F64, F64 with NULLs, two CODE -- one "
             f"with its text on the device --, two more I64) and {n_groups:,} groups.  Per count and round: the keeping remove and the "
             "keeping append of the same documents, then the dropping remove and append, each followed by `set_columns` + "
             "`set_column_text` + `set_groups` of host arrays already prepared.  Milliseconds, median (min-max); one untimed round first.", ""]
    hx = npa.MmapIndex.synth(spec)
    rows = []
    try:
        a = hx.export()
        hx.reserve(max(args.counts), max(args.counts) * args.doc_len)
        set_prepared(hx, sch, gids, n_groups)
        rng = np.random.default_rng(7)
        for c in args.counts:
            ids = np.sort(rng.choice(n, c, replace=False)).astype(np.int64)
            keep = np.ones(n, bool)
            keep[ids] = False
            new = tokens_of(a, ids)
            new_rows = api.AppendRows(columns={k: v[ids] for k, v in values.items()}, groups=gids[ids], n_groups=n_groups)
            t = {k: [] for k in ("keep remove", "keep append", "drop remove", "drop remove setters", "drop append", "drop append setters",
                                 "kernel", "bytes")}
            for r in range(args.rounds + 1):
                print(f"[attach_time] {c} documents: round {r}", flush=True)
                sch_0 = hx.schema
                out = C.c_int64(0)
                with CapturedStderr() as cap:   # the library calls alone: the mirror's bookkeeping of its own row arrays is host work
                    t0 = time.perf_counter()
                    api._check(api.lib().np_hip_index_remove_keep(hx._h, ids.ctypes.data, ids.size, C.byref(out)))
                    t1 = time.perf_counter()
                api._check(api.lib().np_hip_index_info(hx._h, C.byref(hx._info)))
                hx.schema = sch_0.shrunk(keep)
                dl = np.ascontiguousarray(new[0], np.int64)
                plan = hx._plan_rows(new_rows, c)
                t2 = time.perf_counter()
                hx._append_arrays_rows(dl, new[1], new[2], new_rows, plan)
                t3 = time.perf_counter()
                # the dropping way, from the same state: the host arrays are ready before the clock starts
                sch_a, g_a = hx.schema, hx.get_groups()
                sch_b, g_b = sch_a.shrunk(keep), g_a[keep]
                sch_c = sch_b.extended({k: v[ids] for k, v in values.items()})[0]
                g_c = np.concatenate([g_b, g_a[ids]])
                t4 = time.perf_counter()
                hx.remove_ids(ids)
                t5 = time.perf_counter()
                set_prepared(hx, sch_b, g_b, n_groups)
                t6 = time.perf_counter()
                hx.append_arrays(*new)
                t7 = time.perf_counter()
                set_prepared(hx, sch_c, g_c, n_groups)
                t8 = time.perf_counter()
                if r:
                    m = KERNEL.search(cap.text)
                    for k, v in (("keep remove", t1 - t0), ("keep append", t3 - t2), ("drop remove", t5 - t4), ("drop remove setters", t6 - t5),
                                 ("drop append", t7 - t6), ("drop append setters", t8 - t7)):
                        t[k].append(v)
                    if m:
                        t["kernel"].append(float(m.group(1))), t["bytes"].append(float(m.group(2)))
            rows.append((c, t))
    finally:
        hx.close()
    head = ["documents", "keeping remove", "dropping remove + setters", "ratio", "keeping append", "dropping append + setters", "ratio",
            "compaction kernels", "GB/s (share of the copy rate)"]
    lines.append("| " + " | ".join(head) + " |")
    lines.append("|" + "---|" * len(head))
    for c, t in rows:
        dr = [x + y for x, y in zip(t["drop remove"], t["drop remove setters"])]
        da = [x + y for x, y in zip(t["drop append"], t["drop append setters"])]
        rate = statistics.median([b / s for b, s in zip(t["bytes"], t["kernel"]) if s > 0]) if t["kernel"] else 0.0
        lines.append(f"| {c:,} | {spread(t['keep remove'])} | {spread(dr)} | {statistics.median(dr) / statistics.median(t['keep remove']):.1f}x | "
                     f"{spread(t['keep append'])} | {spread(da)} | {statistics.median(da) / statistics.median(t['keep append']):.1f}x | "
                     f"{spread(t['kernel']) if t['kernel'] else '-'} | {rate / 1e9:.0f} ({rate / COPY_RATE:.2f}) |")
    lines.append("\nThe compaction kernels' time is the select pass, all columns and the groups together (device events around the "
                 "launches); their bytes are the keep bitmap and ranks, the source ids written once and read per array, every surviving "
                 "row read and written once and the validity words.  The dropping way does not count the host's own work of "
                 "renumbering and coding the rows again, which a service would also pay.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:   # what is measured so far is kept, whatever the comparison below meets
        f.write("\n".join(lines) + "\n")
    if args.parent_lib:
        plain_against_parent(args, lines)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
