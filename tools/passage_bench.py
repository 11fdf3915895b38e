#!/usr/bin/env python3
"""Passage retrieval from the entity graph on the GPU, timed next to the route a user had before it.  GPU only,
one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is
started behind a hang).

The two graphs of tools/ppr_bench.py (the planted-partition edge list and the duplicate-group graph), each with a synthetic
mention map of as many chunks as vertices: chunk c mentions d - 1 of vertex c's neighbours, the first in index order, and one
uniform entity, d uniform in 1 .. 8 (numpy default_rng(13); a vertex with fewer neighbours gives fewer), weights uniform in
1 .. 8 — locality and a random gather both.  Per graph and batch (1 and 256 queries of five random seeds):
  * EntityGraph.rank_chunks with 20 iterations and top_k 10, answers left on the device; ms per call by the method of DESIGN
    4.10d — host clock around calls ending in a synchronise, two warm-up calls, the median of three windows of >= 0.25 s;
  * the projection alone (rarc_ppr_chunks) and the projection with its top-k, each between two events, and one rarc_ppr_step
    on the same graph and batch (20 steps from a fresh seed between two events, divided by 20): the projection requests about
    nnz rows of 8 B bytes against the step's 2 m + 4 n, and that ratio is stated beside the ratio of the times (requested bytes
    are not HBM bytes);
  * the route without it: personalized_pagerank(top_k=None) to the host, a float64 sparse product (scipy.sparse where scipy
    imports, else np.add.at), np.argpartition — one timed run per batch.

    python3 tools/passage_bench.py --out profiles/passage_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from louvain_bench import make_rows, planted_edges, step  # noqa: E402
from ppr_bench import windows  # noqa: E402

MENTION_SEED = 13


def synthetic_mentions(n, edges, seed=MENTION_SEED):
    """-> (mentions int64 [nnz][2], weights int64 [nnz]) over n chunks and n entities, as the module docstring says"""
    rng = np.random.default_rng(seed)
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    order = np.lexsort((dst, src))
    src, dst = src[order], dst[order]
    start = np.searchsorted(src, np.arange(n))
    rank = np.arange(len(src)) - start[src]                       # position of a neighbour in its vertex's sorted row
    d = rng.integers(1, 9, n)
    keep = rank < (d - 1)[src]
    near = np.stack([src[keep], dst[keep]], axis=1)
    far = np.stack([np.arange(n), rng.integers(0, n, n)], axis=1)
    mentions = np.concatenate([near, far]).astype(np.int64)
    return mentions, rng.integers(1, 9, len(mentions)).astype(np.int64)


def host_route(g, sd, mentions, weights, n, iterations, top_k):
    """what a user did before rank_chunks: the [B][n] scores to the host, a float64 sparse product, argpartition"""
    t0 = time.perf_counter()
    scores = g.personalized_pagerank(sd, max_iterations=iterations)          # float64 [B][n] on the host
    t1 = time.perf_counter()
    try:
        import scipy.sparse as sp

        A = sp.csr_matrix((weights.astype(np.float64), (mentions[:, 0], mentions[:, 1])), shape=(n, n))
        how = "scipy.sparse csr @ dense, float64"
        t2 = time.perf_counter()
        chunk = np.asarray(A @ scores.T)
    except ImportError:
        how = "numpy np.add.at over the mentions, float64"
        t2 = time.perf_counter()
        chunk = np.zeros((n, scores.shape[0]))
        np.add.at(chunk, mentions[:, 0], weights[:, None] * scores.T[mentions[:, 1]])
    top = np.argpartition(-chunk, top_k, axis=0)[:top_k]
    t3 = time.perf_counter()
    return {"seconds": round((t1 - t0) + (t3 - t2), 4), "scores_to_host_seconds": round(t1 - t0, 4),
            "product_and_partition_seconds": round(t3 - t2, 4), "how": how, "checksum": int(top.sum())}


def bench_graph(torch, lib, B, PG, PS, name, n, pairs_dev, edges_host, a):
    g = PG.EntityGraph(n, pairs_dev)
    m = g.m
    mentions, weights = step(f"{name}-mentions", 300, lambda: synthetic_mentions(n, edges_host))
    mm = step(f"{name}-map", 300, lambda: PS.MentionMap(n, n, mentions, weights))
    rng = np.random.default_rng(11)
    res = {"vertices": n, "edges": m, "chunks": n, "mentions": mm.nnz, "split_chunks": mm.n_split, "iterations": a.iterations,
           "top_k": a.top_k, "batches": {}}
    for nq in (1, 256):
        seeds = rng.integers(0, n, (nq, 5))
        sd = torch.from_numpy(seeds).to(g.device)
        run = lambda: g.rank_chunks(mm, sd, max_iterations=a.iterations, top_k=a.top_k, as_device=True)      # noqa: E731
        entry = {"call": step(f"{name}-call-{nq}", 300, lambda: windows(torch, run))}
        vertices = lambda: g.personalized_pagerank(sd, max_iterations=a.iterations, top_k=a.top_k, as_device=True)      # noqa: E731
        entry["vertex_call"] = step(f"{name}-vertex-call-{nq}", 300, lambda: windows(torch, vertices))
        run()                                                     # the state of this call stays in both workspaces
        ws, gb, cws = g._ws, g._graph, mm._cws
        st = torch.cuda.current_stream(g.device).cuda_stream
        ids = torch.empty((nq, a.top_k), dtype=torch.int64, device=g.device)
        sc = torch.empty((nq, a.top_k), dtype=torch.float64, device=g.device)
        cnt = torch.empty(nq, dtype=torch.int32, device=g.device)

        def project():
            B.check(lib.rarc_ppr_chunks(n, m, nq, 0, ws.data_ptr(), ws.numel(), mm._row_ptr.data_ptr(), mm._ent.data_ptr(), mm._w.data_ptr(),
                                        n, mm.nnz, mm._split.data_ptr() if mm._split is not None else None, mm.n_split, cws.data_ptr(),
                                        cws.numel(), st), "rarc_ppr_chunks")

        def topk():
            B.check(lib.rarc_ppr_chunks_topk(n, nq, a.top_k, cws.data_ptr(), cws.numel(), ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), st),
                    "rarc_ppr_chunks_topk")

        wd = torch.ones((nq, 5), dtype=torch.int32, device=g.device)

        def seeded_steps():
            """`iterations` steps from a fresh seed between two events (a step repeated on the same state would find delta = 0
            and freeze every query) -> ms per step"""
            B.check(lib.rarc_ppr_seed(gb.data_ptr(), gb.numel(), n, m, sd.data_ptr(), wd.data_ptr(), nq, 5, ws.data_ptr(), ws.numel(), st),
                    "rarc_ppr_seed")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cur = 0
            for _ in range(a.iterations):
                B.check(lib.rarc_ppr_step(gb.data_ptr(), gb.numel(), n, m, nq, 55706, 0, cur, ws.data_ptr(), ws.numel(), None, st), "rarc_ppr_step")
                cur ^= 1
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.iterations

        def between_events(fn, repeats=10):
            out = []
            for _ in range(repeats + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                out.append(e0.elapsed_time(e1))
            return round(statistics.median(out[2:]), 4)
        entry["projection_ms"] = step(f"{name}-project-{nq}", 120, lambda: between_events(project))
        entry["projection_and_topk_ms"] = step(f"{name}-tail-{nq}", 120, lambda: between_events(lambda: (project(), topk())))
        entry["step_ms"] = round(statistics.median(step(f"{name}-step-{nq}", 120, lambda: [seeded_steps() for _ in range(5)][2:])), 4)
        rows_projection, rows_step = mm.nnz + n, 2 * m + 4 * n              # rows of 8 B bytes requested: gathered + written
        entry["requested_row_ratio_projection_to_step"] = round(rows_projection / rows_step, 4)
        entry["time_ratio_projection_to_step"] = round(entry["projection_ms"] / entry["step_ms"], 4)
        entry["tail_in_steps"] = round(entry["projection_and_topk_ms"] / entry["step_ms"], 2)
        entry["host_route"] = step(f"{name}-host-{nq}", 900, lambda: host_route(g, sd, mentions, weights, n, a.iterations, a.top_k))
        res["batches"][str(nq)] = entry
        print(json.dumps({name: {str(nq): entry}}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database.graph_db import pagerank as PG
    from rag_arc_amd.encapsulation.database.graph_db import passages as PS
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "limits": PS.limits(), "mention_seed": MENTION_SEED,
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; "
                     "projection, projection + top-k: one launch sequence between two events, median of 10 after 2 warm-ups; step: 20 steps from a fresh seed "
                     "between two events / 20, median of 3 after 2 warm-ups"}

    edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
    res["planted_partition"] = bench_graph(torch, lib, B, PG, PS, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges, a)
    del edges
    torch.cuda.empty_cache()

    x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
    pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
    pairs = pairs[:found].contiguous()
    del x
    res["duplicate_groups"] = bench_graph(torch, lib, B, PG, PS, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy(), a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
