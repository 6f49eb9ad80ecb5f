"""Times np_hip_maxsim_batch (maxsim_scores on device tensors: f32, bf16, f16, int8, binary and int4 document rows) against rerank_maxsim
called once per query and against torch (matmul + amax + sum on the device), and quantize_rows / pack_rows_b1 / quantize_rows_i4 against a
device-to-device copy of their input bytes, alternating in one process, and writes profiles/maxsim_time.md.

    python tools/maxsim_time.py [--rounds 5] [--out profiles/maxsim_time.md] [--long-only]

The last section times np_hip_maxsim_batch_long and np_hip_maxsim_batch_long_i8 (maxsim/maxsim_long.py) on queries past 256
tokens beside torch, and a 256-token call through both entries; --long-only times that section alone and replaces it in --out.

Call time is device-synchronised wall time; a window repeats a call until it is at least 0.2 s long (after a warm-up
call).  FLOP/s = 2 * query tokens * document tokens * dim per pair; bytes/s = ALL rows of the call's arrays once plus the
scores (listed shapes read fewer documents than that).  These are call figures, not kernel figures: a maxsim_batch call
includes maxsim_scores' packing of the pair lists and its host-to-device copies of the offsets and ids."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "next-plaid_amd"), ROOT]
import next_plaid_amd as npa  # noqa: E402
from maxsim import maxsim_b1 as B1  # noqa: E402
from maxsim import maxsim_f16 as F16  # noqa: E402
from maxsim import maxsim_i4 as I4  # noqa: E402
from maxsim import maxsim_long as ML  # noqa: E402

# (name, queries, query tokens, documents, document tokens, dim, listed documents per query or None = all pairs)
SHAPES = [("64 x 1000 listed x 300 tok, dim 128", 64, 32, 4000, 300, 128, 1000),
          ("32 x 32 all pairs, 1030-tok pages, dim 128", 32, 24, 32, 1030, 128, None),
          ("16 x 200 listed x 300 tok, dim 1024", 16, 32, 800, 300, 1024, 200)]
# all pairs, large enough that the document bytes matter: int8, binary and int4 rows only, made on the device
BIG = ("64 x 20000 all pairs, 1030-tok pages, dim 128", 64, 32, 20000, 1030, 128)


def window(fn, sync):
    fn(); sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn(); sync()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= 0.2:
            return dt / n


LONG_HEAD = "## np_hip_maxsim_batch_long: queries past 256 tokens, and what the pass loop costs at 256"
# (name, queries, query tokens, documents, document tokens, dim, listed documents per query or None, also through np_hip_maxsim_batch)
LONG_SHAPES = [("32 x 32 all pairs, 1030-tok pages against 1030-tok pages, dim 128", 32, 1030, 32, 1030, 128, None, False),
               ("8 x 200 listed x 300 tok, 2048-tok queries, dim 128", 8, 2048, 800, 300, 128, 200, False),
               ("64 x 1000 listed x 300 tok, 256-tok queries, dim 128", 64, 256, 4000, 300, 128, 1000, True)]
# int8 rows through np_hip_maxsim_batch_long_i8, and the other ways to score the same codes: widened (code * scale) to bf16
# through np_hip_maxsim_batch_long -- the only way for a long query without the entry -- and, at 256 tokens, np_hip_maxsim_batch_i8
LONG_I8 = "maxsim_batch_long_i8 int8 rows (+ f32 row scales)"
LONG_I8_OTHERS = ("maxsim_batch_long the int8 rows widened to bf16, precision 3", "maxsim_batch int8 rows (+ f32 row scales)")


def long_section(rounds, sync):
    """maxsim_scores_long on device tensors beside torch's einsum -> amax -> sum on the same tensors; the 256-token shape goes
    through api.maxsim_scores too (the same bits): the difference is what the pass loop and one query per workgroup cost.
    The same rows quantised to int8 go through maxsim_scores_long_i8, beside those codes widened to bf16 through maxsim_scores_long."""
    import torch
    lines = ["", LONG_HEAD, "",
             "The protocol above: one process, %d alternating rounds, call times.  torch = per query `einsum('dtk,qk->dtq')`," % rounds,
             "`amax(1)`, `sum(1)` on the same device tensors.", "",
             "| shape | path | ms | spread ms | TFLOP/s |", "|---|---|---|---|---|"]
    notes = ["", "The int8 entry against the other ways to score the same codes (medians of the table):"]
    g = np.random.default_rng(2)
    for name, B, lq, nd, ld, dim, k, both in LONG_SHAPES:
        tq = torch.from_numpy(g.standard_normal((B * lq, dim)).astype(np.float32)).cuda()
        td = torch.from_numpy(g.standard_normal((nd * ld, dim)).astype(np.float32)).cuda()
        hq, hd = tq.to(torch.bfloat16), td.to(torch.bfloat16)
        qoff, doff = np.arange(B + 1) * lq, np.arange(nd + 1) * ld
        pairs = None if k is None else [g.choice(nd, k, replace=False) for _ in range(B)]
        idx = None if pairs is None else torch.from_numpy(np.stack(pairs)).cuda()
        flop = 2.0 * B * (nd if k is None else k) * lq * ld * dim

        def call(fn, x, y, prec):
            return lambda: fn(x, y, pairs=pairs, precision=prec, query_offsets=qoff, document_offsets=doff)

        def torch_ref(x, y3):
            def f():
                for b in range(B):
                    torch.einsum("dtk,qk->dtq", y3 if idx is None else y3[idx[b]], x[b * lq:(b + 1) * lq]).amax(1).sum(1)
            return f
        paths = []
        for label, x, y, prec in (("f32, precision 0", tq, td, 0), ("bf16 rows, precision 3", hq, hd, 3), ("f32 rows, precision 3", tq, td, 3)):
            paths.append(("maxsim_batch_long " + label, call(ML.maxsim_scores_long, x, y, prec)))
            if both:
                paths.append(("maxsim_batch " + label, call(npa.maxsim_scores, x, y, prec)))
        (cq, sq), (cd, sd) = npa.quantize_rows(tq), npa.quantize_rows(td)
        wq, wd = ((c.float() * s[:, None]).to(torch.bfloat16) for c, s in ((cq, sq), (cd, sd)))
        i8 = dict(pairs=pairs, query_offsets=qoff, document_offsets=doff)
        paths += [(LONG_I8, lambda: ML.maxsim_scores_long_i8(cq, cd, sq, sd, **i8)),
                  (LONG_I8_OTHERS[0], call(ML.maxsim_scores_long, wq, wd, 3))]
        if both:
            paths.append((LONG_I8_OTHERS[1], lambda: npa.maxsim_scores(cq, cd, query_scales=sq, document_scales=sd, **i8)))
        paths += [("torch f32 einsum+amax+sum", torch_ref(tq, td.view(nd, ld, dim))),
                  ("torch bf16 einsum+amax+sum", torch_ref(hq, hd.view(nd, ld, dim)))]
        times = {p[0]: [] for p in paths}
        for _ in range(rounds):
            for pname, fn in paths:
                times[pname].append(window(fn, sync))
        for pname, _ in paths:
            t = np.array(times[pname])
            lines.append(f"| {name} | {pname} | {np.median(t) * 1e3:.3f} | {t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f} | {flop / np.median(t) / 1e12:.2f} |")
        a = np.array(times[LONG_I8]) * 1e3
        for other in LONG_I8_OTHERS:
            if other in times:
                b = np.array(times[other]) * 1e3
                notes.append(f"- {name}: {np.median(a):.3f} ms against {np.median(b):.3f} ms of `{other}`: {abs(np.median(a) / np.median(b) - 1) * 100:.1f} % "
                             f"{'faster' if np.median(a) < np.median(b) else 'SLOWER'}; the two spreads (max - min) are {np.ptp(a):.3f} and {np.ptp(b):.3f} ms.")
    return lines + notes + ["", "Not measured: kernel time apart from call time; any LDS budget of the int8 kernel other than its 80 KB; the LDS bank",
                            "conflicts of its fragment reads; int8 rows at any dim but 128."]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_time.md"))
    ap.add_argument("--long-only", action="store_true", help="time only the long-query section and replace it in --out")
    a = ap.parse_args()
    sync = torch.cuda.synchronize
    if a.long_only:
        kept = open(a.out).read().split("\n" + LONG_HEAD)[0].rstrip("\n").split("\n")
        lines = kept + long_section(a.rounds, sync)
        open(a.out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines[len(kept):]))
        return
    lines = ["# np_hip_maxsim_batch against rerank_maxsim per query and torch", "",
             "Median call time over %d alternating rounds (min .. max), device-synchronised.  Call figures, not kernel" % a.rounds,
             "figures: maxsim_batch includes the Python packing of the pair lists and the copies of offsets and ids; bytes count",
             "every row of the call's arrays once, also where a list names only some documents.", "",
             "| shape | path | ms | spread ms | TFLOP/s | GB/s |", "|---|---|---|---|---|---|"]
    g = np.random.default_rng(1)
    for name, B, lq, nd, ld, dim, k in SHAPES:
        q = g.standard_normal((B * lq, dim)).astype(np.float32)
        d = g.standard_normal((nd * ld, dim)).astype(np.float32)
        qoff, doff = np.arange(B + 1) * lq, np.arange(nd + 1) * ld
        pairs = None if k is None else [g.choice(nd, k, replace=False) for _ in range(B)]
        npairs = B * (nd if k is None else k)
        flop = 2.0 * npairs * lq * ld * dim
        tq, td = torch.from_numpy(q).cuda(), torch.from_numpy(d).cuda()
        hq, hd = tq.to(torch.bfloat16), td.to(torch.bfloat16)
        fq, fd = tq.to(torch.float16), td.to(torch.float16)
        (cq, sq), (cd, sd) = npa.quantize_rows(tq), npa.quantize_rows(td)
        bd, sb = B1.pack_rows_b1(td)
        wd, sw = I4.quantize_rows_i4(td)
        td3 = td.view(nd, ld, dim)
        idx = None if pairs is None else torch.from_numpy(np.stack(pairs)).cuda()

        def ours(x, y, prec):
            return lambda: npa.maxsim_scores(x, y, pairs=pairs, precision=prec, query_offsets=qoff, document_offsets=doff)

        def ours_i8():
            return npa.maxsim_scores(cq, cd, pairs=pairs, query_offsets=qoff, document_offsets=doff, query_scales=sq, document_scales=sd)

        def ours_f16():
            return F16.maxsim_scores_f16(fq, fd, pairs=pairs, query_offsets=qoff, document_offsets=doff)

        def ours_b1():
            return B1.maxsim_scores_b1(cq, sq, bd, sb, pairs=pairs, query_offsets=qoff, document_offsets=doff)

        def ours_i4():
            return I4.maxsim_scores_i4(cq, sq, wd, sw, pairs=pairs, query_offsets=qoff, document_offsets=doff)

        def torch_ref(x, y3):
            def f():
                for b in range(B):      # one query at a time keeps the [docs, lq, ld] intermediate small
                    docs = y3 if idx is None else y3[idx[b]]
                    (docs @ x[b * lq:(b + 1) * lq].T).amax(1).sum(1)
            return f

        def rerank():
            for b in range(B):
                ids = range(nd) if pairs is None else pairs[b]
                npa.rerank_maxsim(q[b * lq:(b + 1) * lq], [d[i * ld:(i + 1) * ld] for i in ids])
        paths = [("maxsim_batch f32, precision 0", ours(tq, td, 0), 4), ("maxsim_batch bf16 rows, precision 3", ours(hq, hd, 3), 2),
                 ("maxsim_batch_f16 f16 rows", ours_f16, 2),
                 ("maxsim_batch f32 rows, precision 3", ours(tq, td, 3), 4), ("maxsim_batch int8 rows (+ f32 row scales)", ours_i8, 1),
                 ("maxsim_batch_b1 int8 queries, binary documents (+ f32 row scales)", ours_b1, (1, 1 / 8)),
                 ("maxsim_batch_i4 int8 queries, int4 documents (+ f32 row scales)", ours_i4, (1, 1 / 2)),
                 ("torch f32 matmul+amax+sum", torch_ref(tq, td3), 4), ("torch bf16 matmul+amax+sum", torch_ref(hq, hd.view(nd, ld, dim)), 2),
                 ("rerank_maxsim per query (host arrays)", rerank, 4)]
        times = {p[0]: [] for p in paths}
        for _ in range(a.rounds):
            for pname, fn, _ in paths:
                times[pname].append(window(fn, sync))
        for pname, _, es in paths:
            t = np.array(times[pname])
            esq, esd = es if isinstance(es, tuple) else (es, es)
            byts = q.size * esq + d.size * esd + npairs * 4
            lines.append(f"| {name} | {pname} | {np.median(t) * 1e3:.3f} | {t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f} | "
                         f"{flop / np.median(t) / 1e12:.2f} | {byts / np.median(t) / 1e9:.1f} |")
    name, B, lq, nd, ld, dim = BIG
    cq = torch.randint(-128, 128, (B * lq, dim), dtype=torch.int8, device="cuda")
    cd = torch.randint(-128, 128, (nd * ld, dim), dtype=torch.int8, device="cuda")
    bd = torch.randint(-2 ** 31, 2 ** 31, (nd * ld, dim // 32), dtype=torch.int32, device="cuda")
    wd = torch.randint(-2 ** 31, 2 ** 31, (nd * ld, dim // 8), dtype=torch.int32, device="cuda")
    sq, sd = torch.rand(B * lq, device="cuda") + 0.5, torch.rand(nd * ld, device="cuda") + 0.5
    qoff, doff = np.arange(B + 1) * lq, np.arange(nd + 1) * ld
    paths = [("maxsim_batch int8 rows (+ f32 row scales)",
              lambda: npa.maxsim_scores(cq, cd, query_offsets=qoff, document_offsets=doff, query_scales=sq, document_scales=sd), cd.numel()),
             ("maxsim_batch_b1 int8 queries, binary documents (+ f32 row scales)",
              lambda: B1.maxsim_scores_b1(cq, sq, bd, sd, query_offsets=qoff, document_offsets=doff), bd.numel() * 4),
             ("maxsim_batch_i4 int8 queries, int4 documents (+ f32 row scales)",
              lambda: I4.maxsim_scores_i4(cq, sq, wd, sd, query_offsets=qoff, document_offsets=doff), wd.numel() * 4)]
    times = {p[0]: [] for p in paths}
    for _ in range(a.rounds):
        for pname, fn, _ in paths:
            times[pname].append(window(fn, sync))
    for pname, _, dbytes in paths:
        t = np.array(times[pname])
        lines.append(f"| {name} | {pname} | {np.median(t) * 1e3:.3f} | {t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f} | "
                     f"{2.0 * B * nd * lq * ld * dim / np.median(t) / 1e12:.2f} | {(cq.numel() + dbytes + B * nd * 4) / np.median(t) / 1e9:.1f} |")
    del cd, bd, wd, sd
    lines += ["", "## quantize_rows, pack_rows_b1 and quantize_rows_i4 against a device-to-device copy of the same input bytes", "",
              "GB/s counts the input rows once (the quantiser also writes a quarter (f32) or half (bf16) as many bytes of codes, the packer a",
              "32nd or a 16th as many of bit words, the int4 quantiser an 8th or a quarter as many of nibble words; the copy writes as many",
              "as it reads).", "",
              "| rows x dim, input | path | ms | spread ms | input GB/s |", "|---|---|---|---|---|"]
    for n, dim, dt in ((1 << 20, 128, torch.float32), (1 << 20, 128, torch.bfloat16), (1 << 17, 1024, torch.float32)):
        x = torch.randn((n, dim), device="cuda").to(dt)
        y = torch.empty_like(x)
        paths = [("quantize_rows", lambda: npa.quantize_rows(x)), ("pack_rows_b1", lambda: B1.pack_rows_b1(x)),
                 ("quantize_rows_i4", lambda: I4.quantize_rows_i4(x)),
                 ("torch copy_ (device to device)", lambda: y.copy_(x))]
        times = {p[0]: [] for p in paths}
        for _ in range(a.rounds):
            for pname, fn in paths:
                times[pname].append(window(fn, sync))
        for pname, _ in paths:
            t = np.array(times[pname])
            lines.append(f"| {n} x {dim}, {str(dt).split('.')[-1]} | {pname} | {np.median(t) * 1e3:.3f} | {t.min() * 1e3:.3f} .. {t.max() * 1e3:.3f} | "
                         f"{x.numel() * x.element_size() / np.median(t) / 1e9:.1f} |")
    lines += long_section(a.rounds, sync)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
