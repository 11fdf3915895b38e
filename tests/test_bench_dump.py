"""bench.py --dump-outputs without a GPU: what dump_outputs writes for an answer (ids, scores [nq][k]) — the whole answer up to
64 MB, above that a fixed, seeded sample of whole query rows that is the same on every run of the same shape."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def _answer(torch, nq, k):
    ids = torch.arange(nq * k, dtype=torch.int64).reshape(nq, k) * 7 + 3
    scores = 1.0 - torch.arange(nq * k, dtype=torch.float32).reshape(nq, k) / (nq * k)
    return ids, scores


def test_small_answers_are_written_whole(tmp_path):
    import torch

    bench = _bench()
    ids, scores = _answer(torch, 256, 100)
    bench.dump_outputs(torch, np, str(tmp_path), ids, scores)
    assert sorted(os.listdir(tmp_path)) == ["ids.npy", "scores.npy"]
    got_i, got_s = np.load(tmp_path / "ids.npy"), np.load(tmp_path / "scores.npy")
    assert got_i.dtype == np.float64 and got_s.dtype == np.float32
    assert np.array_equal(got_i, ids.numpy().astype(np.float64)) and np.array_equal(got_s, scores.numpy())


def test_large_answers_are_a_fixed_sample_within_64_mb(tmp_path):
    import torch

    bench = _bench()
    nq, k = 8192, 1000                       # 98 MB as float64 ids + float32 scores
    ids, scores = _answer(torch, nq, k)
    picks = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        bench.dump_outputs(torch, np, str(d), ids, scores)
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        rows = np.load(d / "query_rows.npy")
        assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and rows[0] >= 0 and rows[-1] < nq
        r = rows.astype(np.int64)
        assert len(r) > nq // 2              # as much of the answer as the limit allows, not a token sample
        got_i, got_s = np.load(d / "ids.npy"), np.load(d / "scores.npy")
        assert got_i.shape == got_s.shape == (len(r), k)
        assert np.array_equal(got_i, ids.numpy()[r].astype(np.float64)) and np.array_equal(got_s, scores.numpy()[r])
        picks.append(r)
    assert np.array_equal(picks[0], picks[1])
