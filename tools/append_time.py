#!/usr/bin/env python3
"""Time np_hip_index_append against reload() on synthetic index directories and write profiles/append_time.md.

For each corpus size (documents x 300 tokens, K = 2^16, dim 128, 4 bits) a directory is written once (the corpus is
generated in HBM, exported and written by the library's host writer), opened, and then, in ROUNDS alternating rounds per batch
size: reload() of the directory is timed, then one append_arrays of the batch with a prior reserve() and one without (their
order alternates from round to round).  NP_APPEND_TRACE=1 makes the library print each stage's seconds and the merge
kernel's own time (device events) to stderr, which is captured per call.  One untimed reload and append per batch size come
first (code objects, pinned staging).  Needs an MI355X; there is no fallback.

    python tools/append_time.py --out profiles/append_time.md [--sizes 100000 1000000] [--rounds 3] [--work DIR]
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
os.environ["NP_APPEND_TRACE"] = "1"

import numpy as np  # noqa: E402

import next_plaid_amd as npa  # noqa: E402
from next_plaid_amd import synth  # noqa: E402

STAGES = ["grow", "upload + token stages", "distinct-code rebuild", "posting-list merge", "range table"]
COPY_RATE = 6.29e12   # bytes/s of a float4 copy measured on the MI355X (the micro-architecture guide's HBM figure)
LINE = re.compile(r"\[np append\] (.+?)\s+([0-9.]+) s(?:\s+(\d+) entries (\d+) new)?")


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
    return spec


def timed_append(hx, lens, codes, res):
    with CapturedStderr() as cap:
        t0 = time.perf_counter()
        hx.append_arrays(lens, codes, res)
        total = time.perf_counter() - t0
    out = {"total": total}
    for name, sec, entries, new in LINE.findall(cap.text):
        out[name.strip()] = float(sec)
        if entries:
            out["entries"], out["new"] = int(entries), int(new)
    return out


def spread(xs):
    return f"{statistics.median(xs) * 1e3:.1f} ({min(xs) * 1e3:.1f}-{max(xs) * 1e3:.1f})"


def measure(n_docs, args, work, lines):
    path = os.path.join(work, f"ix_{n_docs}")
    t0 = time.perf_counter()
    spec = write_directory(path, n_docs, args.doc_len, args.centroids, args.dim, args.nbits, seed=1236)
    lines.append(f"\n## {n_docs:,} documents x {args.doc_len} tokens\n")
    lines.append(f"Directory written in {time.perf_counter() - t0:.1f} s (generated in HBM, exported, host writer).\n")
    print(f"[append_time] {n_docs} documents: directory written", flush=True)
    # the batches: documents of the same generator beyond the corpus, encoded already (codes + residuals in file geometry)
    big = synth.SynthSpec(num_docs=n_docs + max(args.batches), num_centroids=args.centroids, dim=args.dim, nbits=args.nbits,
                          doc_len_min=args.doc_len, doc_len_max=args.doc_len, seed=spec.seed)
    batches = {}
    for b in args.batches:
        codes, res, lens = synth.doc_tokens(big, n_docs, n_docs + b)
        batches[b] = (lens, codes, res)
    hx = npa.MmapIndex.load(path)
    reloads, rows = [], {(b, m): [] for b in args.batches for m in ("reserved", "unreserved")}
    try:
        for b in args.batches:   # warm-up, untimed
            hx.reload()
            hx.reserve(b, b * args.doc_len)
            hx.append_arrays(*batches[b])
            hx.append_arrays(*batches[b])
        for r in range(args.rounds):
            print(f"[append_time] {n_docs} documents: round {r}", flush=True)
            for b in args.batches:
                t0 = time.perf_counter()
                hx.reload()
                reloads.append(time.perf_counter() - t0)
                for mode in (("reserved", "unreserved") if r % 2 == 0 else ("unreserved", "reserved")):
                    if mode == "reserved":
                        hx.reserve(b, b * args.doc_len)
                    rows[b, mode].append(timed_append(hx, *batches[b]))
    finally:
        hx.close()
    shutil.rmtree(path, ignore_errors=True)
    lines.append(f"`reload()`: median {spread(reloads)} ms over {len(reloads)} calls.\n")
    lines.append("Milliseconds, median (min-max) over the rounds; the stages are the library's own marks (each ends in a device "
                 "synchronise), `total` is the host clock around `append_arrays`.\n")
    lines.append("| batch | reserve | total | " + " | ".join(STAGES) + " | merge kernel | merge GB/s | share of copy rate | reload / total |")
    lines.append("|---|---|---|" + "---|" * (len(STAGES) + 4))
    med_reload = statistics.median(reloads)
    for (b, mode), ms in rows.items():
        cells = [spread([m["total"] for m in ms])] + [spread([m.get(s, 0.0) for m in ms]) for s in STAGES]
        k = [m for m in ms if m.get("merge kernel", 0) > 0]
        if k:
            # the kernel reads every old entry (4 B) and every new pair (8 B) once and writes every entry (4 B)
            rates = [(8.0 * m["entries"] + 4.0 * m["new"]) / m["merge kernel"] for m in k]
            cells += [spread([m["merge kernel"] for m in k]), f"{statistics.median(rates) / 1e9:.0f}",
                      f"{statistics.median(rates) / COPY_RATE:.2f}"]
        else:
            cells += ["-", "-", "-"]
        cells.append(f"{med_reload / statistics.median([m['total'] for m in ms]):.1f}x")
        lines.append(f"| {b:,} | {mode} | " + " | ".join(cells) + " |")
    return {b: med_reload / statistics.median([m["total"] for m in rows[b, "reserved"]]) for b in args.batches}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_time.md"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--batches", type=int, nargs="+", default=[300, 3000, 30000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--doc-len", type=int, default=300)
    ap.add_argument("--centroids", type=int, default=65536)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nbits", type=int, default=4)
    ap.add_argument("--work", default=None, help="directory for the synthetic index directories (default: a temporary one)")
    ap.add_argument("--notes", default=None, help="a file whose text is appended to the profile (e.g. the bench comparison)")
    args = ap.parse_args()
    if npa.device_count() < 1:
        raise SystemExit("append_time.py needs a gfx950 GPU: a time is a GPU measurement or it is not one")
    work = args.work or tempfile.mkdtemp(prefix="np_append_")
    os.makedirs(work, exist_ok=True)
    lines = ["# Appending to a resident index against reloading it", "",
             f"`python tools/append_time.py --sizes {' '.join(map(str, args.sizes))} --rounds {args.rounds}` on one MI355X: "
             f"K = {args.centroids}, dim {args.dim}, {args.nbits} bits, documents of {args.doc_len} tokens; per batch size and round one "
             "`reload()`, one `append_arrays` after `reserve()` and one without, their order alternating between rounds; one untimed "
             "reload and two untimed appends per batch size first.  The claim checked: at a fixed batch the reserved append follows the "
             "appended tokens plus one pass over the posting lists and the codes, not the residuals, so it lies below `reload()`."]
    ratios = {}
    for n in args.sizes:
        try:
            ratios[n] = measure(n, args, work, lines)
        except (MemoryError, OSError) as e:   # a size that does not fit this machine's memory or disk: say so, keep what
            # was measured.  Anything else -- a device error above all -- ends the run: nothing more is started on that GPU
            lines.append(f"\n## {n:,} documents: NOT MEASURED ({type(e).__name__}: {e})\n")
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    lines.append("\n## reload() over reserved append (medians)\n")
    for n, r in ratios.items():
        lines.append(f"- {n:,} documents: " + ", ".join(f"{b:,} new: {x:.1f}x" for b, x in r.items()))
    if args.notes and os.path.exists(args.notes):
        lines.append("\n" + open(args.notes).read().rstrip())
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if not args.work:
        shutil.rmtree(work, ignore_errors=True)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
