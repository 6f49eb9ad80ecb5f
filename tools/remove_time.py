#!/usr/bin/env python3
"""Time np_hip_index_remove against reload() on synthetic index directories and write profiles/remove_time.md.

For each corpus size (documents x 300 tokens, K = 2^16, dim 128, 4 bits) a directory is written once (the corpus is generated
in HBM, exported and written by the library's host writer) and opened.  Then, in ROUNDS alternating rounds, for every count
(300 / 3 000 / 30 000) and place (random, the front, the end): reload() of the untouched directory -- timed, and what brings the
handle back to the whole corpus -- and one remove_ids of the documents.  NP_REMOVE_TRACE=1 makes the library print each stage's
seconds and the two kernels' own times (device events) to stderr, which is captured per call.  One untimed reload and remove per
case come first (code objects).  Last, the directory delete of the largest random case is applied in place and timed, and
reload() of the rewritten directory -- what a delete costs without this entry -- is timed ROUNDS times.  The slab candidates
(--slabs) are timed on the largest front case, where every token moves.  Needs an MI355X; there is no fallback.

    python tools/remove_time.py --out profiles/remove_time.md [--sizes 100000 1000000] [--rounds 3] [--work DIR]
"""
import argparse
import os
import re
import shutil
import statistics
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
from next_plaid_amd import synth  # noqa: E402

STAGES = ["survivors", "codes beside", "distinct-code rebuild", "posting-list filter", "range table", "token move", "swap"]
COPY_RATE = 6.29e12   # bytes/s of a float4 copy measured on the MI355X (the micro-architecture guide's HBM figure)
LINE = re.compile(r"\[np remove\] (.+?)\s+([0-9.]+) s(?:\s+(\d+) (entries|tokens) (\d+) (kept|bytes each))?")


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


def write_directory(path, n_docs, doc_len, K, dim, nbits, seed):
    spec = synth.SynthSpec(num_docs=n_docs, num_centroids=K, dim=dim, nbits=nbits, doc_len_min=doc_len, doc_len_max=doc_len,
                           seed=seed)
    cen = synth.centroids(spec)
    cut, wts = synth.bucket_tables(spec)
    hx = npa.MmapIndex.synth(spec, centroids=cen)
    try:
        a = hx.export()
    finally:
        hx.close()
    npa.write_index_dir(path, cen, wts, a["doc_lengths"], a["codes"], a["residuals"], nbits, bucket_cutoffs=cut,
                        cluster_threshold=0.3, chunk_docs=50_000)


def timed_remove(hx, ids):
    with CapturedStderr() as cap:
        t0 = time.perf_counter()
        hx.remove_ids(ids)
        total = time.perf_counter() - t0
    out = {"total": total}
    for name, sec, n, unit, m, what in LINE.findall(cap.text):
        name = name.strip()
        out[name] = float(sec)
        if unit == "entries":
            out["entries"], out["kept"] = int(n), int(m)
        elif unit == "tokens":
            out[name + " tokens"], out["bytes per token"] = int(n), int(m)
    return out


def spread(xs):
    return f"{statistics.median(xs) * 1e3:.1f} ({min(xs) * 1e3:.1f}-{max(xs) * 1e3:.1f})"


def rate_cells(ms):
    """bytes per second of the posting-list pass (it reads every old entry twice -- count and placement -- and writes the kept
    ones: 4 B each) and of the token move (every moved token read and written once; twice when staged), against the copy rate"""
    cells = []
    k = [m for m in ms if m.get("filter kernel", 0) > 0]
    if k:
        r = statistics.median([(8.0 * m["entries"] + 4.0 * m["kept"]) / m["filter kernel"] for m in k])
        cells += [spread([m["filter kernel"] for m in k]), f"{r / 1e9:.0f} ({r / COPY_RATE:.2f})"]
    else:
        cells += ["-", "-"]
    for kind, passes in (("direct", 2.0), ("staged", 4.0)):
        name = f"move kernel {kind}"
        k = [m for m in ms if m.get(name, 0) > 0 and m.get(name + " tokens", 0) > 0]
        if k:
            r = statistics.median([passes * m[name + " tokens"] * m["bytes per token"] / m[name] for m in k])
            cells += [spread([m[name] for m in k]), f"{r / 1e9:.0f} ({r / COPY_RATE:.2f})"]
        else:
            cells += ["-", "-"]
    return cells


def measure(n_docs, args, work, lines):
    path = os.path.join(work, f"ix_{n_docs}")
    t0 = time.perf_counter()
    write_directory(path, n_docs, args.doc_len, args.centroids, args.dim, args.nbits, seed=1236)
    lines.append(f"\n## {n_docs:,} documents x {args.doc_len} tokens\n")
    lines.append(f"Directory written in {time.perf_counter() - t0:.1f} s (generated in HBM, exported, host writer).\n")
    print(f"[remove_time] {n_docs} documents: directory written", flush=True)
    rng = np.random.default_rng(7)
    cases = {}
    for c in args.counts:
        c = min(c, n_docs // 2)
        cases[c, "random"] = np.sort(rng.choice(n_docs, c, replace=False)).astype(np.int64)
        cases[c, "front"] = np.arange(c, dtype=np.int64)
        cases[c, "end"] = np.arange(n_docs - c, n_docs, dtype=np.int64)
    hx = npa.MmapIndex.load(path)
    reloads, rows, slab_rows = [], {k: [] for k in cases}, {}
    try:
        for k, ids in cases.items():   # warm-up, untimed
            hx.remove_ids(ids)
            hx.reload()
        for r in range(args.rounds):
            print(f"[remove_time] {n_docs} documents: round {r}", flush=True)
            for k in (list(cases) if r % 2 == 0 else list(cases)[::-1]):
                rows[k].append(timed_remove(hx, cases[k]))
                t0 = time.perf_counter()
                hx.reload()
                reloads.append(time.perf_counter() - t0)
        big_front = (max(c for c, _ in cases), "front")
        for slab in args.slabs:
            slab_rows[slab] = []
            for r in range(args.rounds):
                hx.tune("remove_slab", slab)
                slab_rows[slab].append(timed_remove(hx, cases[big_front]))
                hx.reload()
        print(f"[remove_time] {n_docs} documents: the directory delete", flush=True)
        big_random = (max(c for c, _ in cases), "random")
        t0 = time.perf_counter()
        npa.api.delete_from_index_dir(path, cases[big_random])
        t_delete = time.perf_counter() - t0
        after = []
        for r in range(args.rounds):
            t0 = time.perf_counter()
            hx.reload()
            after.append(time.perf_counter() - t0)
    finally:
        hx.close()
    shutil.rmtree(path, ignore_errors=True)
    lines.append(f"`reload()` of the untouched directory, alternating with the removes: median {spread(reloads)} ms over {len(reloads)} "
                 f"calls.  `np_hip_index_delete` of {big_random[0]:,} random documents (host only, paid by both ways of persisting a "
                 f"delete): {t_delete:.1f} s; `reload()` of the directory it wrote: median {spread(after)} ms over {len(after)} calls.\n")
    lines.append("Milliseconds, median (min-max) over the rounds; the stages are the library's own marks (each ends in a device "
                 "synchronise), `total` is the host clock around `remove_ids`; kernel columns are device events, with GB/s "
                 "(share of the device's copy rate) beside them.\n")
    head = ["removed", "where", "total"] + STAGES + ["filter kernel", "GB/s", "move direct", "GB/s", "move staged", "GB/s", "reload / total"]
    lines.append("| " + " | ".join(head) + " |")
    lines.append("|" + "---|" * len(head))
    med_reload = statistics.median(after)
    for (c, where), ms in rows.items():
        cells = [spread([m["total"] for m in ms])] + [spread([m.get(s, 0.0) for m in ms]) for s in STAGES] + rate_cells(ms)
        cells.append(f"{med_reload / statistics.median([m['total'] for m in ms]):.1f}x")
        lines.append(f"| {c:,} | {where} | " + " | ".join(cells) + " |")
    if slab_rows:
        lines.append(f"\nThe slab size (`np_hip_index_tune` \"remove_slab\", tokens; the staging buffer is that many residual rows) on "
                     f"{big_front[0]:,} documents removed at the front -- every remaining token moves:\n")
        lines.append("| remove_slab | total | token move | move direct | GB/s | move staged | GB/s |")
        lines.append("|---|---|---|---|---|---|---|")
        for slab, ms in slab_rows.items():
            lines.append(f"| {slab:,} | {spread([m['total'] for m in ms])} | {spread([m.get('token move', 0.0) for m in ms])} | "
                         + " | ".join(rate_cells(ms)[2:]) + " |")
    return {k: med_reload / statistics.median([m["total"] for m in ms]) for k, ms in rows.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remove_time.md"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--counts", type=int, nargs="+", default=[300, 3000, 30000])
    ap.add_argument("--slabs", type=int, nargs="*", default=[1 << 18, 1 << 20, 1 << 21, 1 << 23])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--work", default=None, help="directory for the synthetic index directories (default: a temporary one)")
    ap.add_argument("--notes", default=None, help="a file whose text is appended to the profile (e.g. the unchanged paths' comparison)")
    args = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("remove_time.py needs a gfx950 GPU: a time is a GPU measurement or it is not one")
    work = args.work or tempfile.mkdtemp(prefix="np_remove_")
    os.makedirs(work, exist_ok=True)
    lines = ["# Removing from a resident index against reloading it", "",
             f"`python tools/remove_time.py --sizes {' '.join(map(str, args.sizes))} --rounds {args.rounds}` on one MI355X: "
             f"K = {args.centroids}, dim {args.dim}, {args.nbits} bits, documents of {args.doc_len} tokens; per case and round one "
             "`remove_ids` and one `reload()` of the untouched directory (it restores the handle), the cases' order reversed every "
             "other round; one untimed remove and reload per case first.  `reload / total` divides the median `reload()` of the "
             "directory that the directory delete wrote -- what a delete costs the handle without this entry -- by the remove's median."]
    ratios = {}
    for n in args.sizes:
        try:
            ratios[n] = measure(n, args, work, lines)
        except (MemoryError, OSError) as e:   # a size that does not fit this machine's memory or disk: say so, keep what
            # was measured.  Anything else -- a device error above all -- ends the run: nothing more is started on that GPU
            lines.append(f"\n## {n:,} documents: NOT MEASURED ({type(e).__name__}: {e})\n")
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lines.append("\n## reload() over remove_ids (medians)\n")
    for n, r in ratios.items():
        lines.append(f"- {n:,} documents: " + ", ".join(f"{c:,} {where}: {x:.1f}x" for (c, where), x in r.items()))
    if args.notes and os.path.exists(args.notes):
        lines.append("\n" + open(args.notes).read().rstrip())
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not args.work:
        shutil.rmtree(work, ignore_errors=True)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
