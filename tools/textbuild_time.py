#!/usr/bin/env python3
"""Times the keyword-index build on the device (np_hip_text_build) beside the SQLite path it replaces.

  timeout 1500 python tools/textbuild_time.py      # writes profiles/textbuild_time.md, prints one JSON line per measurement

Corpus: seeded, generated here (nothing is read from anywhere): --docs documents (default 300 000) of about --words words
(default 100, uniform in words/2 .. 3 words/2), drawn with Zipf weights 1 / rank from a fixed vocabulary of --vocab words
(letters and digits, mixed case); trigram runs on a tenth of the documents.  Per tokenizer, in a child process of its own under
its own time limit (a step that fails or runs out of time ends the tool):
    sqlite      TextIndexData.from_texts: the FTS5 inserts plus the fts5vocab read into arrays, ONCE (a CPU yardstick, minutes long)
    equal       the device's arrays are compared with SQLite's, array for array, before anything is timed
    device      api.text_build on the encoded corpus (upload, every stage, read-back of the arrays), wall-clock around the call:
                median (min - max) of --repeats calls after --warmup untimed ones; the stages are the library's own report of
                the median call (host wall-clock around each stage, which ends in a synchronise)
    end to end  TextIndexData.from_texts_device once: the same plus the encoding of the texts and the list of Python terms

  timeout 1500 python tools/textbuild_time.py --utf8 [--parent-lib OLD.so]     # writes profiles/textbuild_utf8_time.md

--utf8 times the UTF-8 mode (utf8=True: unicode61 beyond ASCII from text.unicode61_table) in ONE child process, alternating
rounds: on the same corpus with about one word in ten carrying an accent, from_texts_device with utf8=True (equal to SQLite
and without a fallback document, checked first) beside utf8=False, which sends nearly every document through SQLite; on the
ASCII corpus api.text_build with and without the table, which is the price of the table walk; the probe of the table per
plane; and, given --parent-lib (a libnextplaid_hip.so built from the commit before), the default np_hip_text_build of the two
libraries in alternating rounds on the ASCII corpus.
No ratio is asserted anywhere: the table is what was measured.  What else ran on the machine is not known to the tool; the
spread of the device samples is the evidence there is."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "next-plaid_amd"))


ACCENTS = str.maketrans("aeiouncAEIOU", "áéíöüñçÀÉÎÖÜ")


def make_corpus(n_docs, words, vocab, seed, accent=0.0):
    """accent: the share of the words that carry one (their first letter that has an accented form is replaced); the
    draws come last, so the words and separators are those of the ASCII corpus."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789", np.uint8)
    voc = set()
    while len(voc) < vocab:
        voc.add(bytes(rng.choice(alphabet, int(rng.integers(2, 11)))).decode())
    voc = np.asarray(sorted(voc))
    rng.shuffle(voc)
    w = 1.0 / np.arange(1, vocab + 1)
    cdf = np.cumsum(w / w.sum())
    lens = rng.integers(words // 2, words + words // 2 + 1, n_docs)
    idx = np.minimum(np.searchsorted(cdf, rng.random(int(lens.sum()))), vocab - 1)
    seps = np.asarray([" ", " ", " ", ", ", ". ", "\n", " - "])
    sep = seps[rng.integers(0, len(seps), idx.size)]
    picked = voc[idx]
    if accent > 0:
        def one_accent(w):
            for i, ch in enumerate(w):
                if ch.translate(ACCENTS) != ch:
                    return w[:i] + ch.translate(ACCENTS) + w[i + 1:]
            return w
        acc = np.asarray([one_accent(w) for w in voc.tolist()])
        picked = np.where(rng.random(idx.size) < accent, acc[idx], picked)
    out, at = [], 0
    for n in lens:
        out.append("".join(np.char.add(picked[at: at + n], sep[at: at + n]).tolist()))
        at += n
    return out


def _encode(texts):
    raws = [t.encode() for t in texts]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    return np.frombuffer(b"".join(raws), np.uint8), off


def _stat(ms):
    ms = sorted(ms)
    return {"median": round(ms[len(ms) // 2], 1), "min": round(ms[0], 1), "max": round(ms[-1], 1), "n": len(ms)}


def utf8_child(args):
    """Everything --utf8 measures, in this one process; prints one JSON object."""
    import ctypes as C
    import next_plaid_amd as npa
    from next_plaid_amd import api, text as T
    from next_plaid_amd.text import TextIndexData
    if npa.device_count() < 1:
        raise SystemExit("textbuild_time.py needs a gfx950 GPU: there is nothing to time without one")
    t0 = time.perf_counter()
    table = T.unicode61_table(2)
    out = {"docs": args.docs, "table_s": round(time.perf_counter() - t0, 2),
           "probe_s_per_plane": {str(k): round(v, 3) for k, v in sorted(T.unicode61_probe_seconds.items())}}
    plain = make_corpus(args.docs, args.words, args.vocab, 7)
    accented = make_corpus(args.docs, args.words, args.vocab, 7, accent=0.1)
    out["accented_docs_with_a_byte_above_7f"] = sum(1 for t in accented if not t.isascii())
    # the accented corpus: equal to SQLite first, then alternating rounds
    t0 = time.perf_counter()
    want = TextIndexData.from_texts(accented)
    out["accented_sqlite_s"] = round(time.perf_counter() - t0, 2)
    on, fb = [], []
    for i in range(args.fallback_rounds + 1):
        t0 = time.perf_counter()
        got = TextIndexData.from_texts_device(accented, utf8=True)
        on.append(1e3 * (time.perf_counter() - t0))
        if i == 0:
            assert got.fallback_docs == [] and got.terms == want.terms and got.n_rows == want.n_rows
            for k in ("term_offsets", "inst_doc", "inst_pos"):
                assert np.array_equal(getattr(got, k), getattr(want, k)), k
            out.update(accented_MB=round(sum(len(t.encode()) for t in accented) / 1e6, 1), accented_instances=int(want.inst_doc.size),
                       accented_terms=want.n_terms)
        t0 = time.perf_counter()
        off_ = TextIndexData.from_texts_device(accented)
        fb.append(1e3 * (time.perf_counter() - t0))
        if i == 0:
            assert off_.terms == want.terms and np.array_equal(off_.inst_doc, want.inst_doc)
            out["accented_fallback_docs_without_utf8"] = len(off_.fallback_docs)
    out["accented_utf8_on_ms"], out["accented_utf8_off_ms"] = _stat(on[1:]), _stat(fb[1:])     # (the first round warms up)
    raw_a, off_a = _encode(accented)
    core = []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        r = api.text_build(raw_a, off_a, api.NP_TOK_UNICODE61, utf8=True)
        if i >= args.warmup:
            core.append((1e3 * (time.perf_counter() - t0), r["report"]))
    core.sort(key=lambda x: x[0])
    out["accented_text_build_ms"] = _stat([c[0] for c in core])
    out["accented_stages_ms"] = {k[3:]: round(core[len(core) // 2][1][k], 1) for k in
                                 ("ms_upload", "ms_classify", "ms_emit", "ms_terms", "ms_sort", "ms_total")}
    # the ASCII corpus: the table walk's price
    raw_p, off_p = _encode(plain)
    a = api.text_build(raw_p, off_p, api.NP_TOK_UNICODE61)
    b = api.text_build(raw_p, off_p, api.NP_TOK_UNICODE61, utf8=True)
    assert a["fallback_docs"].size == 0 and b["fallback_docs"].size == 0
    for k in ("term_bytes", "term_byte_offsets", "term_offsets", "inst_doc", "inst_pos"):
        assert np.array_equal(a[k], b[k]), k
    on, offm, on_walk, off_walk = [], [], [], []
    for i in range(args.warmup + args.repeats):
        for utf8, ms, walk in ((False, offm, off_walk), (True, on, on_walk)):
            t0 = time.perf_counter()
            r = api.text_build(raw_p, off_p, api.NP_TOK_UNICODE61, utf8=utf8)
            if i >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
                walk.append(r["report"]["ms_classify"] + r["report"]["ms_emit"] + r["report"]["ms_terms"])
    out.update(ascii_MB=round(raw_p.size / 1e6, 1), ascii_utf8_on_ms=_stat(on), ascii_utf8_off_ms=_stat(offm),
               ascii_walk_and_terms_on_ms=_stat(on_walk), ascii_walk_and_terms_off_ms=_stat(off_walk))
    # the default entry of this library beside the parent commit's, alternating
    if args.parent_lib:
        libs = {"parent": C.CDLL(os.path.abspath(args.parent_lib)), "this": api.lib()}
        ms = {k: [] for k in libs}
        for L in libs.values():
            L.np_hip_text_build.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(api.np_text_build_opts),
                                            C.POINTER(C.c_void_p), C.POINTER(api.np_text_build_report)]
            L.np_hip_text_build_free.argtypes = [C.c_void_p]
            L.np_hip_text_build_free.restype = None
        for i in range(args.warmup + 2 * args.repeats):
            for name, L in libs.items():
                o, rep_, h = api.np_text_build_opts(0), api.np_text_build_report(), C.c_void_p()
                t0 = time.perf_counter()
                rc = L.np_hip_text_build(0, raw_p.ctypes.data, off_p.ctypes.data, off_p.size - 1, C.byref(o), C.byref(h), C.byref(rep_))
                dt = 1e3 * (time.perf_counter() - t0)
                assert rc == 0 and rep_.n_fallback == 0
                L.np_hip_text_build_free(h)
                if i >= args.warmup:
                    ms[name].append(dt)
        out["default_entry_ms"] = {k: _stat(v) for k, v in ms.items()}
    print(json.dumps(out), flush=True)


def utf8_main(args):
    cmd = [sys.executable, os.path.abspath(__file__), "--utf8-child"] + [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in
                                                                          ("docs", "words", "vocab", "repeats", "warmup", "fallback_rounds")]
    if args.parent_lib:
        cmd.append(f"--parent-lib={args.parent_lib}")
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
    if p.returncode != 0:
        raise SystemExit(f"--utf8: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
    r = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(r), flush=True)
    path = args.out
    os.makedirs(os.path.dirname(path), exist_ok=True)
    fmt = lambda s: f"{s['median']} ({s['min']} - {s['max']}, n = {s['n']})"
    with open(path, "w") as f:
        f.write("# unicode61 beyond ASCII on the device: what `utf8=True` costs and saves\n\n")
        f.write("Written by `tools/textbuild_time.py --utf8` (its docstring says what is measured), one process, alternating rounds; "
                f"milliseconds are median (min - max) of wall-clock samples.  {r['docs']} documents of about {args.words} Zipf words over "
                f"a vocabulary of {args.vocab}; the accented corpus is the same corpus with about one word in ten carrying an accent "
                f"({r['accented_docs_with_a_byte_above_7f']} of its documents hold a byte above 0x7F).  What else ran on the machine is not "
                "known to the tool; the spreads are the evidence there is.  No threshold is asserted.\n\n")
        f.write("## The accented corpus (" + f"{r['accented_MB']} MB, {r['accented_instances']} instances, {r['accented_terms']} terms)\n\n")
        f.write("`utf8=True` equalled `TextIndexData.from_texts` (SQLite) array for array with an empty fallback list before anything was timed.\n\n")
        f.write("| path | ms |\n|---|---|\n")
        f.write(f"| `from_texts_device(utf8=True)`: encode, device build, read-back, Python terms | {fmt(r['accented_utf8_on_ms'])} |\n")
        f.write(f"| `from_texts_device()` (utf8=False): {r['accented_fallback_docs_without_utf8']} documents fall back to SQLite and are merged on the host | "
                f"{fmt(r['accented_utf8_off_ms'])} |\n")
        f.write(f"| `api.text_build(utf8=True)` alone (upload, all stages, read-back) | {fmt(r['accented_text_build_ms'])} |\n")
        f.write(f"| `TextIndexData.from_texts` (SQLite), once | {round(1e3 * r['accented_sqlite_s'])} |\n\n")
        s = r["accented_stages_ms"]
        f.write(f"Stages of the median `api.text_build(utf8=True)` call, ms: upload {s['upload']}, classify + scan {s['classify']}, emit {s['emit']}, "
                f"terms {s['terms']}, sort + gather {s['sort']}, total {s['total']}.\n\n")
        f.write(f"## The ASCII corpus ({r['ascii_MB']} MB): the price of the table walk\n\n")
        f.write("The two calls returned the same bytes.  `api.text_build`, alternating:\n\n| | utf8=False | utf8=True |\n|---|---|---|\n")
        f.write(f"| whole call, ms | {fmt(r['ascii_utf8_off_ms'])} | {fmt(r['ascii_utf8_on_ms'])} |\n")
        f.write(f"| classify + emit + terms (the stages that read text), ms | {fmt(r['ascii_walk_and_terms_off_ms'])} | {fmt(r['ascii_walk_and_terms_on_ms'])} |\n\n")
        f.write("## The table\n\n")
        f.write("`text.unicode61_table(2)` probed from SQLite, once per process: " +
                ", ".join(f"plane {k}: {v} s" for k, v in r["probe_s_per_plane"].items()) + f"; the whole call {r['table_s']} s.\n")
        if "default_entry_ms" in r:
            d = r["default_entry_ms"]
            f.write("\n## The default entry beside the parent commit's library\n\n")
            f.write("`np_hip_text_build` without a table on the ASCII corpus, the two libraries loaded into one process, alternating rounds:\n\n")
            f.write(f"| library | ms |\n|---|---|\n| parent commit | {fmt(d['parent'])} |\n| this commit | {fmt(d['this'])} |\n")


def one(args):
    import next_plaid_amd as npa
    from next_plaid_amd import api
    from next_plaid_amd.text import TextIndexData
    if npa.device_count() < 1:
        raise SystemExit("textbuild_time.py needs a gfx950 GPU: there is nothing to time without one")
    tok = args.one
    n_docs = args.docs if tok == "unicode61" else max(args.docs // 10, 1)
    texts = make_corpus(n_docs, args.words, args.vocab, 7)
    raws = [t.encode() for t in texts]
    off = np.zeros(len(raws) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in raws])
    raw = np.frombuffer(b"".join(raws), np.uint8)
    t0 = time.perf_counter()
    want = TextIndexData.from_texts(texts, tok)
    sqlite_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    got = TextIndexData.from_texts_device(texts, tok)
    e2e_s = time.perf_counter() - t0
    assert got.fallback_docs == [] and got.terms == want.terms and got.n_rows == want.n_rows
    for k in ("term_offsets", "inst_doc", "inst_pos"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    code = api.NP_TOK_TRIGRAM if tok == "trigram" else api.NP_TOK_UNICODE61
    runs = []
    for i in range(args.warmup + args.repeats):
        t0 = time.perf_counter()
        r = api.text_build(raw, off, code)
        if i >= args.warmup:
            runs.append((1e3 * (time.perf_counter() - t0), r["report"]))
    runs.sort(key=lambda x: x[0])
    med_ms, rep = runs[len(runs) // 2]
    row = {"tokenizer": tok, "docs": n_docs, "MB": round(raw.size / 1e6, 1), "instances": int(want.inst_doc.size),
           "terms": want.n_terms, "sqlite_s": round(sqlite_s, 2), "device_ms": round(med_ms, 1), "device_ms_min": round(runs[0][0], 1),
           "device_ms_max": round(runs[-1][0], 1), "repeats": args.repeats, "end_to_end_s": round(e2e_s, 2),
           "stages_ms": {k[3:]: round(rep[k], 1) for k in ("ms_upload", "ms_classify", "ms_emit", "ms_terms", "ms_sort", "ms_total")},
           "sort_passes": rep["sort_passes"], "hash_bits": rep["hash_bits"], "table_retries": rep["table_retries"],
           "workspace_MB": round(rep["workspace_bytes"] / 1e6, 1)}
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=300_000)
    ap.add_argument("--words", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--step-timeout", type=int, default=900, help="seconds one tokenizer's child process may take")
    ap.add_argument("--out", default=None, help="default: profiles/textbuild_time.md, with --utf8 profiles/textbuild_utf8_time.md")
    ap.add_argument("--one", choices=["unicode61", "trigram"], help=argparse.SUPPRESS)
    ap.add_argument("--utf8", action="store_true", help="time the UTF-8 mode instead (profiles/textbuild_utf8_time.md)")
    ap.add_argument("--fallback-rounds", type=int, default=2, help="--utf8: timed rounds of the accented corpus (each runs SQLite once)")
    ap.add_argument("--parent-lib", default="", help="--utf8: a libnextplaid_hip.so of the commit before, timed beside this one")
    ap.add_argument("--utf8-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "textbuild_utf8_time.md" if args.utf8 else "textbuild_time.md")
    if args.one:
        return one(args)
    if args.utf8_child:
        return utf8_child(args)
    if args.utf8:
        return utf8_main(args)
    rows = []
    for tok in ("unicode61", "trigram"):
        cmd = [sys.executable, os.path.abspath(__file__), "--one", tok] + [f"--{k}={getattr(args, k)}" for k in
                                                                          ("docs", "words", "vocab", "repeats", "warmup")]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)   # its own time limit; no retry
        if p.returncode != 0:
            raise SystemExit(f"{tok}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-4000:]}")
        rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# The keyword index built on the device beside SQLite's FTS5\n\n")
        f.write("Written by `tools/textbuild_time.py` (its docstring says what each column is).  Zipf words over a fixed vocabulary of "
                f"{args.vocab}; about {args.words} words a document.  The device's arrays equalled SQLite's before anything was timed.  "
                "Device: wall-clock around `api.text_build` (upload, all stages, read-back), median (min - max) of "
                f"{args.repeats} calls after {args.warmup} warm-up; SQLite: `TextIndexData.from_texts`, once, on the same machine in the "
                "same run.  Stages are the library's report of the median call.\n\n")
        f.write("| tokenizer | documents | MB | instances | terms | SQLite s | device ms: median (min - max) | from_texts_device s | "
                "upload | classify + scan | emit | terms | sort + gather | passes | table bits (retries) | device MB |\n")
        f.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            s = r["stages_ms"]
            f.write(f"| {r['tokenizer']} | {r['docs']} | {r['MB']} | {r['instances']} | {r['terms']} | {r['sqlite_s']} | "
                    f"{r['device_ms']} ({r['device_ms_min']} - {r['device_ms_max']}) | {r['end_to_end_s']} | {s['upload']} | "
                    f"{s['classify']} | {s['emit']} | {s['terms']} | {s['sort']} | {r['sort_passes']} | "
                    f"{r['hash_bits']} ({r['table_retries']}) | {r['workspace_MB']} |\n")


if __name__ == "__main__":
    main()
