#!/usr/bin/env python3
"""Times the resident keyword index (np_hip_index_set_text_build, np_hip_index_text_merge) beside the host path it replaces.

  timeout 1100 python tools/text_resident_time.py [--parent-lib PATH]   # writes profiles/text_resident_time.md, one JSON line per row

Corpus: tools/textmerge_time.py's -- the seeded Zipf corpus of --docs documents (default 300 000, unicode61) plus a tenth as
many further documents to append and replace with -- and then a tenth of it.  One process per corpus; inside it the two paths
ALTERNATE, round by round (host then resident in even rounds, resident then host in odd ones), --rounds rounds after one
untimed round.  A figure is the median (min - max) of the rounds; the spread of a row is max - min of the slower-varying path.
    build     MmapIndex.build_text(texts) against build_text(texts, resident=True): wall-clock around the call
    update    MmapIndex.update_text (TextIndexData.updated + set_text, the parent commit's path) against
              update_text(resident=True), for appends of 0.1 %, 1 % and 10 % of the corpus, a 1 % renumbering delete and a 1 %
              replace.  Every timed call starts from the same base: the handle's keyword index is set again, untimed, before it
    append    MmapIndex.append_arrays(rows=AppendRows(texts=...)) of 0.1 %, 1 % and 10 % with a host and with a resident keyword
              index on the handle; the appended documents are removed and the base set again, untimed, before every call
    stages    the merge report of the median resident update, and the bytes the install and the merge read and write over their
              time beside the device's copy rate (a device-to-device copy of 256 MB through torch, median of 5)
Before anything is timed the resident result is compared with the host path's: get_text_layout byte for byte.
With --parent-lib (the library built from the parent commit) np_hip_text_build_merge and np_hip_index_set_text are timed
against it in processes of their own, alternating, because the merge's host code moved: the allowed difference is the spread
of the parent's own rounds; both are written.
No ratio is asserted anywhere: the tables are what was measured."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from textbuild_time import make_corpus   # noqa: E402
from textmerge_time import OPS, plan_op   # noqa: E402

APPENDS = [("append 0.1 %", 0.001), ("append 1 %", 0.01), ("append 10 %", 0.1)]


def med(xs):
    xs = sorted(xs)
    return [round(xs[len(xs) // 2], 2), round(xs[0], 2), round(xs[-1], 2)]


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def alternate(rounds, host, resident):
    """host() and resident() each return ms (and anything else); one untimed round, then `rounds` alternating ones."""
    h, r = [], []
    for i in range(rounds + 1):
        order = (("h", host), ("r", resident)) if i % 2 == 0 else (("r", resident), ("h", host))
        for who, fn in order:
            got = fn()
            if i > 0:
                (h if who == "h" else r).append(got)
    return h, r


def corpus_child(args):
    import next_plaid_amd as npa
    from next_plaid_amd import api, synth
    from next_plaid_amd.text import TextIndexData
    if npa.device_count() < 1:
        raise SystemExit("text_resident_time.py needs a gfx950 GPU: there is nothing to time without one")
    n = args.docs
    allt = make_corpus(n + n // 10, args.words, args.vocab, 7)
    texts, extra = allt[:n], allt[n:]
    spec = synth.SynthSpec(num_docs=n + n // 10, num_centroids=64, dim=64, nbits=4, doc_len_min=1, doc_len_max=2, seed=9)
    a = synth.generate_arrays(spec)
    ix = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"], a["codes"],
                                   a["residuals"], a["nbits"], device=0)
    ref = npa.MmapIndex.from_arrays(a["centroids"], a["bucket_weights"], a["ivf"], a["ivf_lengths"], a["doc_lengths"], a["codes"],
                                    a["residuals"], a["nbits"], device=0)

    def same_layout(what):
        x, y = ix.get_text_layout(), ref.get_text_layout()
        for k in y:
            assert x[k].tobytes() == y[k].tobytes(), (what, k)

    base = TextIndexData.from_texts_device(texts)
    assert base.fallback_docs == []
    print(json.dumps({"base": {"docs": n, "instances": int(base.inst_doc.size), "terms": base.n_terms}}), flush=True)
    # ---- the device's copy rate
    import torch
    nbytes = 256 << 20
    p, q = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"), torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    ms = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        q.copy_(p)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    del p, q
    torch.cuda.empty_cache()
    copy_gbs = 2 * nbytes / 1e6 / med(ms[1:])[0]      # read + write
    print(json.dumps({"copy": {"MB": nbytes >> 20, "ms": med(ms[1:]), "GBs_read_plus_write": round(copy_gbs, 1)}}), flush=True)

    # ---- build
    ix.build_text(texts, resident=True)
    ref.set_text(base)
    same_layout("build")
    h, r = alternate(args.rounds, lambda: timed(lambda: ix.build_text(texts))[0], lambda: timed(lambda: ix.build_text(texts, resident=True))[0])
    print(json.dumps({"build": {"host_ms": med(h), "resident_ms": med(r)}}), flush=True)

    # ---- update
    for label, kind, frac in OPS:
        op = plan_op(kind, frac, n, extra)
        kw = dict(delete=op["delete"], replace=op["replace"], renumber=True)
        ix.build_text(texts, resident=True)
        ix.update_text(op["new_texts"], resident=True, **kw)
        ref.set_text(base)
        ref.update_text(op["new_texts"], **kw)
        same_layout(label)
        reports = []

        def host():
            ix.set_text(base)
            return timed(lambda: ix.update_text(op["new_texts"], **kw))[0]

        def resident():
            ix.build_text(texts, resident=True)
            ms, data = timed(lambda: ix.update_text(op["new_texts"], resident=True, **kw))
            reports.append((ms, data.build_report))
            return ms

        h, r = alternate(args.rounds, host, resident)
        reports = sorted(reports[1:], key=lambda x: x[0])
        rep = reports[len(reports) // 2][1]
        z = ix.text_sizes()
        # bytes the merge's device work moves at least: A's doc (written, read twice), pos read, the result written, S and keep
        na, nout = rep["n_base_instances"], rep["n_instances"]
        merge_bytes = na * (8 + 8 + 8 + 4 + 4 + 4 + 4) + nout * 12
        install_bytes = nout * (8 + 4 + 4 + 4 + 4) + z["n_postings"] * (4 + 4 + 8 + 8 + 4)
        dev_ms = rep["ms_upload"] + rep["ms_count"] + rep["ms_place"]
        print(json.dumps({"update": {"op": label, "host_ms": med(h), "resident_ms": med(r),
                                     "merge_ms": {k[3:]: round(rep[k], 2) for k in ("ms_check", "ms_upload", "ms_count", "ms_terms", "ms_place", "ms_total")},
                                     "batch_build_ms": round((rep.get("batch") or {}).get("ms_total", 0.0), 2),
                                     "merge_device_GBs": round(merge_bytes / 1e6 / max(dev_ms, 1e-3), 1),
                                     "merge_MB": round(merge_bytes / 1e6, 1), "install_MB": round(install_bytes / 1e6, 1),
                                     "workspace_MB": round(rep["workspace_bytes"] / 1e6, 1)}}), flush=True)

    # ---- append through append_arrays(rows=...)
    T0 = int(a["doc_lengths"][:n].sum())
    ix.close()
    ref.close()
    import importlib.util
    spec_r = importlib.util.spec_from_file_location("remove_restate", os.path.join(ROOT, "tests", "remove_restate.py"))
    RR = importlib.util.module_from_spec(spec_r)
    spec_r.loader.exec_module(RR)
    small = RR.shrunk_arrays(a, np.arange(n, n + n // 10))
    ix = npa.MmapIndex.from_arrays(small["centroids"], small["bucket_weights"], small["ivf"], small["ivf_lengths"], small["doc_lengths"],
                                   small["codes"], small["residuals"], small["nbits"], device=0)
    ix.reserve(n // 10, int(a["doc_lengths"][n:].sum()))
    for label, frac in APPENDS:
        k = max(int(round(n * frac)), 1)
        Tk = int(a["doc_lengths"][n:n + k].sum())
        tail = (a["doc_lengths"][n:n + k], a["codes"][T0:T0 + Tk], a["residuals"][T0:T0 + Tk])
        rows = api.AppendRows(texts=extra[:k])

        def back():
            if ix.num_documents() > n:
                ix.remove_ids(np.arange(n, ix.num_documents()))

        def host():
            back()
            ix.set_text(base)
            return timed(lambda: ix.append_arrays(*tail, rows=rows))[0]

        def resident():
            back()
            ix.build_text(texts, resident=True)
            return timed(lambda: ix.append_arrays(*tail, rows=rows))[0]

        h, r = alternate(args.rounds, host, resident)
        print(json.dumps({"append": {"op": label, "docs": k, "host_ms": med(h), "resident_ms": med(r)}}), flush=True)
    ix.close()


def parent_child(args):
    """np_hip_text_build_merge (append 1 %) and np_hip_index_set_text through the library at --lib, bound by hand: the
    parent's library lacks the new entries, so api.lib() (which binds every entry) cannot load it.  Only the entries the two
    timed calls need are bound; the base's arrays come from this tree's library (TextIndexData.from_texts_device), untimed --
    so where --lib IS this tree's library, the timed instance is the one the base was built in, and the parent's is a fresh one."""
    from next_plaid_amd import api, synth
    from next_plaid_amd.text import TextIndexData
    api._preload_hip_runtime()
    L = C.CDLL(args.lib)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.np_hip_last_error.restype = C.c_char_p
    L.np_hip_index_from_arrays.argtypes = [C.POINTER(api.np_index_arrays), C.POINTER(api.np_open_opts), C.POINTER(vp)]
    L.np_hip_index_close.argtypes = [vp]
    L.np_hip_index_close.restype = None
    L.np_hip_index_set_text.argtypes = [vp, C.POINTER(api.np_text_index)]
    L.np_hip_text_build.argtypes = [i32, vp, vp, i64, C.POINTER(api.np_text_build_opts), C.POINTER(vp), C.POINTER(api.np_text_build_report)]
    L.np_hip_text_build_sizes.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.np_hip_text_build_fetch.argtypes = [vp, vp, vp, vp, vp, vp]
    L.np_hip_text_build_free.argtypes = [vp]
    L.np_hip_text_build_free.restype = None
    L.np_hip_text_build_merge.argtypes = [i32, C.POINTER(api.np_text_index), vp, vp, vp, i64, vp, vp, i64, C.POINTER(api.np_text_merge_opts),
                                          C.POINTER(vp), C.POINTER(api.np_text_merge_report)]

    def ok(rc, what):
        if rc != 0:
            raise SystemExit(f"{what}: rc {rc}: {L.np_hip_last_error().decode(errors='replace')}")

    n = args.docs
    allt = make_corpus(n + n // 10, args.words, args.vocab, 7)
    texts, extra = allt[:n], allt[n:n + max(n // 100, 1)]
    base = TextIndexData.from_texts_device(texts)
    enc = [t.encode() for t in base.terms]
    a_tbo = np.zeros(len(enc) + 1, np.int64)
    a_tbo[1:] = np.cumsum([len(t) for t in enc])
    a_tb = np.frombuffer(b"".join(enc), np.uint8)
    a_off, a_doc, a_pos = (np.ascontiguousarray(x, t) for x, t in ((base.term_offsets, np.int64), (base.inst_doc, np.int64), (base.inst_pos, np.int32)))
    t_base = api.np_text_index(len(enc), a_off.ctypes.data, a_doc.ctypes.data, a_pos.ctypes.data, int(base.n_rows))
    raws = [t.encode() for t in extra]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    raw = np.frombuffer(b"".join(raws), np.uint8)
    remap = np.arange(n, dtype=np.int64)
    ids = n + np.arange(len(raws), dtype=np.int64)
    spec = synth.SynthSpec(num_docs=n + n // 10, num_centroids=64, dim=64, nbits=4, doc_len_min=1, doc_len_max=2, seed=9)
    a = synth.generate_arrays(spec)
    keep = [np.ascontiguousarray(a[k], t) for k, t in (("centroids", np.float32), ("bucket_weights", np.float32), ("ivf", np.int64),
                                                         ("ivf_lengths", np.int32), ("doc_lengths", np.int64), ("codes", np.int64),
                                                         ("residuals", np.uint8))]
    arr = api.np_index_arrays(keep[4].size, 0, keep[4].size, keep[0].shape[0], keep[0].shape[1], int(a["nbits"]),
                              *(x.ctypes.data for x in keep))
    ix, o = vp(), api._opts(device=0)
    ok(L.np_hip_index_from_arrays(C.byref(arr), C.byref(o), C.byref(ix)), "np_hip_index_from_arrays")
    merge, sett = [], []
    for i in range(args.warmup + args.repeats):
        d, h = vp(), vp()
        bo, brep = api.np_text_build_opts(0), api.np_text_build_report()
        ok(L.np_hip_text_build(0, raw.ctypes.data, off.ctypes.data, len(raws), C.byref(bo), C.byref(d), C.byref(brep)), "np_hip_text_build")
        ok(L.np_hip_text_build_sizes(d, None, None, None, None), "np_hip_text_build_sizes")
        mo, rep = api.np_text_merge_opts(0), api.np_text_merge_report()
        ok(L.np_hip_text_build_merge(0, C.byref(t_base), a_tb.ctypes.data, a_tbo.ctypes.data, remap.ctypes.data, remap.size, d,
                                     ids.ctypes.data, n + len(raws), C.byref(mo), C.byref(h), C.byref(rep)), "np_hip_text_build_merge")
        nt, nb, ni, nr = i64(), i64(), i64(), i64()
        ok(L.np_hip_text_build_sizes(h, C.byref(nt), C.byref(nb), C.byref(ni), C.byref(nr)), "np_hip_text_build_sizes")
        r_off, r_doc, r_pos = np.zeros(nt.value + 1, np.int64), np.zeros(ni.value, np.int64), np.zeros(ni.value, np.int32)
        ok(L.np_hip_text_build_fetch(h, None, None, r_off.ctypes.data, r_doc.ctypes.data, r_pos.ctypes.data), "np_hip_text_build_fetch")
        L.np_hip_text_build_free(h)
        L.np_hip_text_build_free(d)
        t_new = api.np_text_index(nt.value, r_off.ctypes.data, r_doc.ctypes.data, r_pos.ctypes.data, nr.value)
        t0 = time.perf_counter()
        ok(L.np_hip_index_set_text(ix, C.byref(t_new)), "np_hip_index_set_text")
        ms2 = 1e3 * (time.perf_counter() - t0)
        if i >= args.warmup:
            merge.append(float(rep.ms_total))
            sett.append(ms2)
    L.np_hip_index_close(ix)
    print(json.dumps({"lib": args.lib, "merge_ms": med(merge)[0], "set_text_ms": med(sett)[0]}), flush=True)


def child(args, *extra, docs=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + list(extra) + [f"--{k}={getattr(args, k)}" for k in
                                                                      ("words", "vocab", "repeats", "warmup", "rounds")]
    cmd.append(f"--docs={docs or args.docs}")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
    if p.returncode != 0:
        raise SystemExit(f"{extra}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
    return [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith("{")]


def fmt(v):
    return f"{v[0]} ({v[1]} - {v[2]})"


def ratio(h, r):
    """host / resident of the medians, and whether the gap exceeds both spreads"""
    gap, spread = h[0] - r[0], max(h[2] - h[1], r[2] - r[1])
    return f"{h[0] / max(r[0], 1e-9):.1f}x" + ("" if gap > spread else " (inside the spread)")


def write_head(f, args):
    f.write("Written by `tools/text_resident_time.py` (its docstring says what each row is).  unicode61; the seeded Zipf corpus of "
            "`tools/textmerge_time.py` and a tenth of it.  Host and resident calls alternate in one process, "
            f"{args.rounds} rounds after one untimed round; every figure is wall-clock milliseconds around the Python call, median "
            "(min - max).  The ratio is host / resident of the medians; it is marked where the gap is inside the larger of the two "
            "spreads.  The resident result's layout equalled the host path's byte for byte before anything was timed.  All on one "
            "machine in one run.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--words", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default="", help="libnextplaid_hip.so built from the parent commit")
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text_resident_time.md"))
    ap.add_argument("--one", choices=["corpus", "parent"], help=argparse.SUPPRESS)
    ap.add_argument("--lib", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one == "corpus":
        return corpus_child(args)
    if args.one == "parent":
        return parent_child(args)
    runs = []
    for docs in (args.docs, max(args.docs // 10, 100)):
        rows = child(args, "--one=corpus", docs=docs)
        for r in rows:
            print(json.dumps(r), flush=True)
        runs.append(rows)
    rounds = []
    if args.parent_lib:
        from next_plaid_amd import api
        libs = {"p": os.path.abspath(args.parent_lib), "t": os.path.abspath(api.library_path())}
        for i in range(args.parent_rounds):
            got = {}
            for who in ("pt" if i % 2 == 0 else "tp"):
                got[who] = child(args, "--one=parent", f"--lib={libs[who]}")[-1]
            rounds.append((got["p"], got["t"]))
            print(json.dumps({"round": len(rounds), "parent": got["p"], "tree": got["t"]}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# The resident keyword index beside the host path\n\n")
        write_head(f, args)
        for rows in runs:
            by = {}
            for r in rows:
                for k, v in r.items():
                    by.setdefault(k, []).append(v)
            b, c = by["base"][0], by["copy"][0]
            f.write(f"\n## {b['docs']} documents, {b['instances']} instances, {b['terms']} terms\n\n")
            f.write(f"Device copy rate: {c['MB']} MB device to device in {fmt(c['ms'])} ms, {c['GBs_read_plus_write']} GB/s read plus write.\n\n")
            f.write("| call | host ms | resident ms | host / resident |\n|---|---|---|---|\n")
            x = by["build"][0]
            f.write(f"| build_text | {fmt(x['host_ms'])} | {fmt(x['resident_ms'])} | {ratio(x['host_ms'], x['resident_ms'])} |\n")
            for x in by["update"]:
                f.write(f"| update_text: {x['op']} | {fmt(x['host_ms'])} | {fmt(x['resident_ms'])} | {ratio(x['host_ms'], x['resident_ms'])} |\n")
            for x in by.get("append", []):
                f.write(f"| append_arrays(rows): {x['op']} ({x['docs']} documents) | {fmt(x['host_ms'])} | {fmt(x['resident_ms'])} | "
                        f"{ratio(x['host_ms'], x['resident_ms'])} |\n")
            f.write("\nThe median resident update's merge report (ms) and the bytes its device work moves at least, over upload + count + "
                    "place:\n\n| operation | batch's build | check | upload (maps, expanding launch) | count | strings | place | merge total | "
                    "merge MB | GB/s | install MB | planned workspace MB |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for x in by["update"]:
                m = x["merge_ms"]
                f.write(f"| {x['op']} | {x['batch_build_ms']} | {m['check']} | {m['upload']} | {m['count']} | {m['terms']} | {m['place']} | "
                        f"{m['total']} | {x['merge_MB']} | {x['merge_device_GBs']} | {x['install_MB']} | {x['workspace_MB']} |\n")
        if rounds:
            f.write("\n## np_hip_text_build_merge and np_hip_index_set_text against the parent commit's library\n\n")
            f.write("The merge's implementation gained a second caller (the resident base) and its messages take the entry's name; "
                    "`np_hip_index_set_text` itself did not move.  The larger corpus, an append of 1 %, "
                    f"{len(rounds)} rounds alternating the parent's library and this tree's (and which goes first), each in a process of "
                    f"its own; a round's figure is the median of {args.repeats} calls after {args.warmup} warm-up: the merge's own "
                    "`ms_total`, and wall-clock around `set_text`.  The allowed difference is the spread of the parent's own rounds.\n\n")
            f.write("| round | parent merge ms | this tree merge ms | parent set_text ms | this tree set_text ms |\n|---|---|---|---|---|\n")
            for i, (p, t) in enumerate(rounds):
                f.write(f"| {i + 1} | {p['merge_ms']} | {t['merge_ms']} | {p['set_text_ms']} | {t['set_text_ms']} |\n")
            for key, name in (("merge_ms", "np_hip_text_build_merge"), ("set_text_ms", "np_hip_index_set_text")):
                ps, ts = [p[key] for p, _ in rounds], [t[key] for _, t in rounds]
                f.write(f"\n{name}: parent median {med(ps)[0]}, spread {round(max(ps) - min(ps), 2)} ({min(ps)} - {max(ps)}); this tree "
                        f"median {med(ts)[0]} ({min(ts)} - {max(ts)}); the medians differ by {round(med(ts)[0] - med(ps)[0], 2)} ms.\n")


if __name__ == "__main__":
    main()
