"""Batched MMR on the MI355X: batch_max_marginal_relevance_search next to the same queries through the single call, one JSON file.

--rows x --dim fp16 rows (seeded normal, metric "cosine") adopted by a HipFlatVectorStore, --nq query texts from a lookup-table
provider, reembed=False.  Per (k, fetch_k) cell: `loop_ms` — max_marginal_relevance_search once per query (one search, a gather,
rarc_mmr_select in one workgroup and a read-back each: the path that has not changed) — and `batch_ms` —
batch_max_marginal_relevance_search for all of them (per 256: one search_device, one rarc_mmr_select_rows, one host mapping) —
with `loop_over_batch`; the two answers are compared document for document first.  Times are host clock around whole calls (both
end in a read-back, so in a synchronised device), after two warm-up calls of the same shape; three windows per entry, the median
reported with the windows' spread (max - min over median).

  python tools/mmr_bench.py --out profiles/mmr_batch_bench.json
  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/mmr_bench.py --batched-only --cells 5 20
      (kernel times: one trace per cell, so that every kernel's average belongs to that cell; tools/mmr_kstats.py sums them)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, target_s=0.5, windows=3, max_reps=50):
    """(median ms per call, spread, calls per window) of fn(): two warm-up calls, then `windows` windows that fill target_s."""
    for _ in range(2):
        fn()
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = int(min(max_reps, max(2, target_s / one)))
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ms.append((time.perf_counter() - t0) / reps * 1e3)
    ms.sort()
    return ms[len(ms) // 2], (ms[-1] - ms[0]) / ms[len(ms) // 2], reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=256)
    ap.add_argument("--cells", type=int, nargs="+", default=[5, 20, 20, 100], help="k fetch_k [k fetch_k ...]")
    ap.add_argument("--batched-only", action="store_true", help="run the batched call alone, ten times per cell (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import torch

    from rag_arc_amd.core.utils.data_model import Document
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from rag_arc_amd.encapsulation.embeddings.table import TableEmbeddings
    from rag_arc_amd.hip.engine import FlatIndexF16

    if not torch.cuda.is_available():
        raise SystemExit("mmr_bench needs a ROCm device: a CPU run measures nothing")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1234)
    idx = FlatIndexF16(args.dim, metric="cosine", device=0)
    for s0 in range(0, args.rows, 100_000):
        idx.add(torch.randn((min(100_000, args.rows - s0), args.dim), generator=gen, device=dev))
    texts = [f"query {i}" for i in range(args.nq)]
    vectors = np.random.default_rng(7).standard_normal((args.nq, args.dim)).astype(np.float32)
    store = HipFlatVectorStore(TableEmbeddings(texts, vectors), metric="cosine")
    store.adopt(idx, [Document(content="", metadata={}, id=str(i)) for i in range(args.rows)])
    cells = []
    for k, fetch_k in zip(args.cells[0::2], args.cells[1::2]):
        batch = lambda: store.batch_max_marginal_relevance_search(texts, k=k, fetch_k=fetch_k, reembed=False)
        loop = lambda: [store.max_marginal_relevance_search(t, k=k, fetch_k=fetch_k, reembed=False) for t in texts]
        if args.batched_only:
            for _ in range(10):
                batch()
            continue
        same = [[d.id for d in a] for a in batch()] == [[d.id for d in a] for a in loop()]
        search_ms, search_spread, _ = timed(lambda: (idx.search_device(vectors, fetch_k), torch.cuda.synchronize(dev)))
        batch_ms, batch_spread, batch_reps = timed(batch)
        loop_ms, loop_spread, loop_reps = timed(loop, max_reps=5)
        cell = {"nq": args.nq, "k": k, "fetch_k": fetch_k, "same_documents": same,
                "batch_ms": round(batch_ms, 3), "batch_spread": round(batch_spread, 3), "batch_calls_per_window": batch_reps,
                "loop_ms": round(loop_ms, 3), "loop_spread": round(loop_spread, 3), "loop_calls_per_window": loop_reps,
                "loop_over_batch": round(loop_ms / batch_ms, 2),
                "search_device_fetch_k_ms": round(search_ms, 3), "search_spread": round(search_spread, 3)}
        cells.append(cell)
        print(json.dumps(cell), flush=True)
        if args.out:            # (rewritten after every cell: a run that is cut short keeps what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                json.dump({"rows": args.rows, "dim": args.dim, "storage": "f16", "metric": "cosine", "reembed": False,
                           "mmr_stats": dict(store.mmr_stats), "cells": cells}, fh, indent=1)
    if not args.batched_only and not all(c["same_documents"] and c["loop_over_batch"] > 1.0 for c in cells):
        raise SystemExit("mmr_bench: the batched call is not faster than the loop in every cell, or answers differ")


if __name__ == "__main__":
    main()
