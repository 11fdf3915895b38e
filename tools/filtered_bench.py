"""Filtered search on the MI355X: both strategies of FlatIndexF16.search_filtered next to the unfiltered search, one JSON file.

--rows x --dim fp16 rows (seeded normal, metric "cosine"), and for every --nq, --k and allowed --share a random row set:
the unfiltered search_device (the yardstick: that code does not change with this feature), then search_filtered_device forced
to "subset" (rarc_search_rows), forced to "overfetch" (search for k' + rarc_strike_rows + fallback) and "auto".  Times are host
clock around `reps` calls that end in a device synchronise, after two warm-up calls of the same shape; three such windows per
entry, the median reported with the windows' spread (max - min over median).  Answers stay on the device: no copy-out in the
timed window.  Per cell: the strategy "auto" took, and auto's time over the faster forced strategy's.

  python tools/filtered_bench.py --nq 1 256 --out profiles/filtered_1m_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, dev, fn, target_s=0.25, windows=3):
    """(median ms per call, spread) of fn(): warm-up, then `windows` windows of enough calls to fill target_s."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    one = max(time.perf_counter() - t0, 1e-6)
    reps = int(min(200, max(3, target_s / one)))
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    ms.sort()
    return ms[len(ms) // 2], (ms[-1] - ms[0]) / ms[len(ms) // 2], reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--share", type=float, nargs="+", default=[0.001, 0.01, 0.1, 0.5])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from rag_arc_amd.hip.engine import FlatIndexF16

    if not torch.cuda.is_available():
        raise SystemExit("filtered_bench needs a ROCm device: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    idx = FlatIndexF16(args.dim, metric="cosine", device=0)
    for s0 in range(0, args.rows, 100_000):
        idx.add(torch.randn((min(100_000, args.rows - s0), args.dim), generator=gen, device=dev))
    rng = np.random.default_rng(7)
    cells = []
    for nq in args.nq:
        q = torch.randn((nq, args.dim), generator=gen, device=dev)
        for k in args.k:
            base_ms, base_spread, _ = timed(torch, dev, lambda: idx.search_device(q, k))
            for share in args.share:
                m = max(1, int(round(args.rows * share)))
                rs = idx.rowset(np.sort(rng.choice(args.rows, m, replace=False)))
                cell = {"nq": nq, "k": k, "share": share, "m": m, "unfiltered_ms": round(base_ms, 4),
                        "unfiltered_spread": round(base_spread, 3), "auto_takes": idx.filter_strategy(nq, k, m)}
                before = dict(idx.filtered_stats)
                for strategy in ("subset", "overfetch", "auto"):
                    ms, spread, reps = timed(torch, dev, lambda: idx.search_filtered_device(q, k, rs, strategy=strategy))
                    cell[strategy + "_ms"], cell[strategy + "_spread"] = round(ms, 4), round(spread, 3)
                cell["fallback_queries"] = idx.filtered_stats["fallback_queries"] - before["fallback_queries"]
                cell["auto_over_best"] = round(cell["auto_ms"] / min(cell["subset_ms"], cell["overfetch_ms"]), 3)
                cells.append(cell)
                print(json.dumps(cell), flush=True)
                if args.out:            # (rewritten after every cell: a run that is cut short keeps what it measured)
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as fh:
                        json.dump({"rows": args.rows, "dim": args.dim, "storage": "f16", "metric": "cosine", "cells": cells}, fh, indent=1)


if __name__ == "__main__":
    main()
