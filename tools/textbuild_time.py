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


def make_corpus(n_docs, words, vocab, seed):
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
    out, at = [], 0
    for n in lens:
        out.append("".join(np.char.add(voc[idx[at: at + n]], sep[at: at + n]).tolist()))
        at += n
    return out


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "textbuild_time.md"))
    ap.add_argument("--one", choices=["unicode61", "trigram"], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
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
