"""`bench.py --dump-outputs DIR`: what the timed path returned in its LAST timed step, as float arrays, equal to the CPU oracle on
that step's query batch.  --steps 5 and --steps 6 end on different batches, so the files follow the step count.  Needs a real MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import RTOL_F32, assert_ranking_close, make_arrays, oracle_index, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, QUERY_BATCHES = 64, 4


def _bench(out, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--docs", "20000", "--doc-len", "120", "--centroids", "4096",
           "--steps", str(steps), "--warmup", "1", "--cpu-queries", "0", "--parity-queries", "0", "--workspace-gib", "1",
           "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_is_the_last_timed_step(tmp_path):
    spec, a = make_arrays(num_docs=20000, num_centroids=4096, dim=128, nbits=4, doc_len_min=120, doc_len_max=120, seed=1236)
    qs, _ = synth.make_queries(spec, BATCH * QUERY_BATCHES, n_tokens=32, cen=a["centroids"])
    ox = oracle_index(a)
    po = O.SearchParameters(n_full_scores=4096, top_k=10, n_ivf_probe=32, centroid_batch_size=100_000, centroid_score_threshold=0.4)
    for steps in (5, 6):
        out = tmp_path / f"s{steps}"
        d = _bench(out, steps)
        assert d["steps"] == steps and d["ms_per_step"] > 0
        # a plain run (no --full) measures nothing beyond the steps and their p50 latency
        assert d["full"] is False and d["p50_batch_latency_ms"] > 0
        assert d["stages"] is d["roofline"] is d["cpu_baseline"] is d["parity_vs_oracle"] is d["value_pcie_inclusive"] is None
        ids, sc, cnt = (np.load(out / f"{n}.npy") for n in ("passage_ids", "scores", "counts"))
        assert ids.dtype == np.float64 and sc.dtype == np.float32 and cnt.dtype == np.float64
        assert ids.shape == sc.shape == (BATCH, 10) and cnt.shape == (BATCH,)
        assert sorted(os.listdir(out)) == ["counts.npy", "passage_ids.npy", "scores.npy"]
        b = (steps - 1) % QUERY_BATCHES                     # bench.py's batch of its last timed step
        ref = ox.search_batch(qs[b * BATCH:(b + 1) * BATCH], po)
        for i, r in enumerate(ref):
            n = int(cnt[i])
            assert n == len(r.passage_ids), (steps, i)
            assert np.all(ids[i, n:] == -1) and np.all(np.isneginf(sc[i, n:]))
            assert_ranking_close(ids[i, :n].astype(np.int64), sc[i, :n], r.passage_ids, r.scores, RTOL_F32, f"steps {steps} q{i}")
