"""`bench.py` without --full on one GPU: the line is the headline alone (no other leg, no full-size check), and
--dump-outputs writes what the timed path answered in its last step — the exact top-k of bench's own synthetic inputs, bit
for bit the CPU oracle's, and the same arrays on every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_the_headline_and_dumps_its_last_answer(tmp_path, oracle):
    n, d, nq, k = 200_000, 768, 256, 100
    env = dict(os.environ)
    for key in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(key, None)
    outs = []
    for run in range(2):
        out_dir = tmp_path / f"run{run}"
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(n), "--steps", "4",
                            "--warmup", "1", "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout[-2000:]
        out = json.loads(lines[0])
        assert out["steps"] == 4 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f16"
        assert out["config"]["n_corpus"] == n and out["config"]["full_size_check"] is None and out["cpu_baseline"] is None
        assert not {"c2", "c3", "c5", "wide", "pairs", "f32", "api", "persistence", "ingest"} & set(out)
        assert sorted(os.listdir(out_dir)) == ["ids.npy", "scores.npy"]
        ids, scores = np.load(out_dir / "ids.npy"), np.load(out_dir / "scores.npy")
        assert ids.dtype == np.float64 and scores.dtype == np.float32 and ids.shape == scores.shape == (nq, k)
        outs.append((ids, scores))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1].view(np.uint32), outs[1][1].view(np.uint32))
    # bench's inputs rebuilt on the host by the oracle's copy of the generator (bit-identical to the device's): corpus seed
    # 1234, queries seed 4321; the canonical fp32 scorer over the fp16 rows, (score desc, id asc)
    rows = oracle.synth_rows_f16(n, d, seed=1234)
    queries = oracle.synth_rows_f32(nq, d, seed=4321)
    ref_ids, ref_scores, _ = oracle.flat_search_f16(rows, oracle.normalize_L2(queries), k)
    ids, scores = outs[0]
    assert np.array_equal(ids, ref_ids.astype(np.float64)), "dumped ids differ from the oracle's top-k"
    assert np.array_equal(scores.view(np.uint32), ref_scores.view(np.uint32)), "dumped scores differ from the oracle's"
