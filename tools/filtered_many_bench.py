"""One filter per query on the MI355X: FlatIndexF16.search_filtered_many next to a loop of one-query filtered searches, one JSON
file.

--rows x --dim fp16 rows (seeded normal, metric "cosine"), --nq queries, each with a random row set OF ITS OWN (--nq distinct
RowSets) that allows --share of the rows; the last cell mixes the shares, query i taking share i mod len(--share).  Per cell:
  grouped     search_filtered_many_device(queries, k, rowsets) — one call for the batch
  loop        search_filtered_device(queries[i:i+1], k, rowsets[i]) for every i — what a batch of distinct filters cost before
              (that method does not change with this feature: its time is the yardstick)
  unfiltered  search_device(queries, k)
Times are host clock around `reps` calls that end in a device synchronise, after two warm-up calls of the same shape; three
such windows per entry: the median, and the windows' spread (max - min over median).  Answers stay on the device.  Per cell:
grouped over loop, and the legs the grouped call took.

  python tools/filtered_many_bench.py --out profiles/filtered_many_1m_bench.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.filtered_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--share", type=float, nargs="+", default=[0.001, 0.01, 0.1])
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from rag_arc_amd.hip.engine import FlatIndexF16

    if not torch.cuda.is_available():
        raise SystemExit("filtered_many_bench needs a ROCm device: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    idx = FlatIndexF16(args.dim, metric="cosine", device=0)
    for s0 in range(0, args.rows, 100_000):
        idx.add(torch.randn((min(100_000, args.rows - s0), args.dim), generator=gen, device=dev))
    rng = np.random.default_rng(7)
    nq, k = args.nq, args.k
    q = torch.randn((nq, args.dim), generator=gen, device=dev)
    base_ms, base_spread, _ = timed(torch, dev, lambda: idx.search_device(q, k))
    by_share = {}
    for share in args.share:        # nq distinct RowSets per share
        m = max(1, int(round(args.rows * share)))
        by_share[share] = [idx.rowset(np.sort(rng.choice(args.rows, m, replace=False))) for _ in range(nq)]
    mixes = [(str(share), by_share[share]) for share in args.share]
    if len(args.share) > 1:
        mixes.append(("mixed", [by_share[args.share[i % len(args.share)]][i] for i in range(nq)]))
    cells = []
    for name, sets in mixes:
        def loop():
            for i in range(nq):
                idx.search_filtered_device(q[i: i + 1], k, sets[i])

        cell = {"nq": nq, "k": k, "share": name, "distinct_filters": len({id(rs) for rs in sets}),
                "m_min": min(rs.m for rs in sets), "m_max": max(rs.m for rs in sets),
                "unfiltered_ms": round(base_ms, 4), "unfiltered_spread": round(base_spread, 3)}
        before = dict(idx.filtered_stats)
        ms, spread, _ = timed(torch, dev, lambda: idx.search_filtered_many_device(q, k, sets))
        mid = dict(idx.filtered_stats)
        cell["grouped_ms"], cell["grouped_spread"] = round(ms, 4), round(spread, 3)
        ms, spread, _ = timed(torch, dev, loop)
        cell["loop_ms"], cell["loop_spread"] = round(ms, 4), round(spread, 3)
        calls = max(1, mid["grouped_calls"] - before["grouped_calls"])
        cell["grouped_legs_per_call"] = {key: round((mid[key] - before[key]) / calls, 2)
                                         for key in ("subset_batches", "overfetch_batches", "fallback_queries")}
        cell["grouped_over_loop"] = round(cell["grouped_ms"] / cell["loop_ms"], 4)
        cells.append(cell)
        print(json.dumps(cell), flush=True)
        if args.out:            # (rewritten after every cell: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump({"rows": args.rows, "dim": args.dim, "storage": "f16", "metric": "cosine", "cells": cells}, fh, indent=1)


if __name__ == "__main__":
    main()
