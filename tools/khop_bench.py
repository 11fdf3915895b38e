#!/usr/bin/env python3
"""k-hop neighbourhoods on the GPU, timed next to the host and next to a PageRank step.  GPU only, one process;
every step runs under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

The two graphs of tools/ppr_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex, and
the duplicate-group graph of --rows x 768 Gaussian rows) and the mention map of tools/passage_bench.py over each (as many chunks
as vertices).  Per graph, hops (2 and 3) and batch (1 and 256 queries of five random seeds):
  * every step alone: after a seed, each rarc_khop_step between two events of its own, the median of the last three of five
    runs; beside it the bytes the step must move — 2 m (4 + 8 W) for the adjacency and the neighbours' frontier words and
    3 n W 8 for the level words of n vertices (seen read, the new level written, seen written where it grew), W = ceil(nq / 64)
    — as a rate and as a fraction of this box's read stream (rarc_stream_read, bench.py's `peak_measured`);
  * rarc_khop_list (max_vertices 4096) and rarc_khop_chunks alone on the state those steps left, each between two events, the
    median of five;
  * EntityGraph.neighbourhood(max_vertices=4096) and .neighbourhood_chunks(top_k=10), answers left on the device: ms per call
    by the method of tools/ppr_bench.py (the `method` string records it);
  * the host route they replace: one frontier product per hop with scipy.sparse where scipy imports, else numpy over the edge
    list, then the sort by (hop, vertex) per query; one timed run per case;
  * at 256 queries, rarc_ppr_step on the same graph in the same run (20 steps between two events, as tools/ppr_bench.py), and
    whether the slowest k-hop step took less time than it.

    python3 tools/khop_bench.py --out profiles/khop_bench.json
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
from passage_bench import synthetic_mentions  # noqa: E402
from ppr_bench import stream_read_peak, windows  # noqa: E402

PPR_STEPS = 20


def host_route(n, edges, seeds, hops, max_vertices):
    """levels by one frontier product per hop, then each query's list by (hop, vertex) -> (seconds, what ran)"""
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    try:
        import scipy.sparse as sp

        A = sp.csr_matrix((np.ones(len(src), np.float32), (dst, src)), shape=(n, n))
        how = "scipy.sparse csr @ sparse frontier per hop, then lexsort per query"
        t0 = time.perf_counter()
        lv = np.full((len(seeds), n), 255, np.uint8)
        rows = np.repeat(np.arange(len(seeds)), seeds.shape[1])
        lv[rows, seeds.ravel()] = 0
        F = sp.csr_matrix((np.ones(rows.size, np.float32), (seeds.ravel(), rows)), shape=(n, len(seeds)))
        for h in range(1, hops + 1):
            R = (A @ F).tocoo()
            new = lv[R.col, R.row] == 255
            lv[R.col[new], R.row[new]] = h
            F = sp.csr_matrix((np.ones(int(new.sum()), np.float32), (R.row[new], R.col[new])), shape=(n, len(seeds)))
    except ImportError:
        how = "numpy frontier matrix over the edge list per hop, then lexsort per query"
        t0 = time.perf_counter()
        lv = np.full((len(seeds), n), 255, np.uint8)
        lv[np.repeat(np.arange(len(seeds)), seeds.shape[1]), seeds.ravel()] = 0
        frontier = lv == 0
        for h in range(1, hops + 1):
            reach = np.zeros_like(frontier)
            for q in range(len(seeds)):
                reach[q, dst[frontier[q, src]]] = True
            frontier = reach & (lv == 255)
            lv[frontier] = h
    for q in range(len(seeds)):
        inside = np.flatnonzero(lv[q] != 255)
        inside[np.lexsort((inside, lv[q][inside]))][:max_vertices]
    return time.perf_counter() - t0, how


def bench_graph(torch, lib, B, PG, PS, KH, name, n, pairs_dev, edges_host, peak, a):
    g = PG.EntityGraph(n, pairs_dev)
    m = g.m
    mentions, weights = synthetic_mentions(n, edges_host)
    mm = PS.MentionMap(n, n, mentions, weights=weights)
    rng = np.random.default_rng(11)
    res = {"vertices": n, "edges": m, "chunks": n, "mentions": mm.nnz, "cases": {}}
    st = torch.cuda.current_stream(g.device).cuda_stream
    gb = g._graph
    for nq in (1, 256):
        seeds = rng.integers(0, n, (nq, 5))
        sd = torch.from_numpy(seeds).to(g.device)
        W = (nq + 63) // 64
        for hops in (2, 3):
            case = f"hops{hops}-nq{nq}"
            entry = {"hops": hops, "queries": nq}

            def seeded_steps():
                """-> ms of each step, one event pair per step"""
                need = int(lib.rarc_khop_workspace_bytes(n, m, nq, hops))
                if getattr(g, "_khop_ws", None) is None or g._khop_ws.numel() < need:
                    g._khop_ws = torch.empty(need, dtype=torch.uint8, device=g.device)
                ws = g._khop_ws
                B.check(lib.rarc_khop_seed(n, m, sd.data_ptr(), nq, 5, hops, ws.data_ptr(), ws.numel(), st), "rarc_khop_seed")
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(hops + 1)]
                ev[0].record()
                for hop in range(1, hops + 1):
                    B.check(lib.rarc_khop_step(gb.data_ptr(), gb.numel(), n, m, nq, hops, hop, ws.data_ptr(), ws.numel(), None, st), "rarc_khop_step")
                    ev[hop].record()
                ev[hops].synchronize()
                return [ev[i].elapsed_time(ev[i + 1]) for i in range(hops)]
            runs = step(f"{name}-{case}-steps", 300, lambda: [seeded_steps() for _ in range(5)][2:])
            per_hop = [statistics.median(r[i] for r in runs) for i in range(hops)]
            moved = 2 * m * (4 + 8 * W) + 3 * n * W * 8
            entry["step_ms"] = [round(x, 4) for x in per_hop]
            entry["step_bytes"] = moved
            entry["step_GBps"] = [round(moved / (x * 1e-3) / 1e9, 1) for x in per_hop]
            entry["step_frac_of_peak_measured"] = [round(moved / (x * 1e-3) / 1e9 / peak, 4) for x in per_hop]
            # the tails alone, on the state the last run left: one launch sequence between two events, the median of five
            ws, (cws, cb), (split, n_split) = g._khop_ws, mm.workspace(nq), mm.split_list()
            decay = KH.default_decay(hops)
            ids = torch.empty((nq, 4096), dtype=torch.int64, device=g.device)
            hp = torch.empty((nq, 4096), dtype=torch.int32, device=g.device)
            cnt = torch.empty(nq, dtype=torch.int32, device=g.device)

            def between_events(fn):
                out = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    out.append(e0.elapsed_time(e1))
                return round(statistics.median(out), 4)
            entry["list_ms"] = step(f"{name}-{case}-list-alone", 120, lambda: between_events(lambda: B.check(lib.rarc_khop_list(
                n, m, nq, hops, 4096, ws.data_ptr(), ws.numel(), ids.data_ptr(), hp.data_ptr(), cnt.data_ptr(), st), "rarc_khop_list")))
            entry["chunks_ms"] = step(f"{name}-{case}-chunks-alone", 120, lambda: between_events(lambda: B.check(lib.rarc_khop_chunks(
                n, m, nq, hops, decay.ctypes.data, ws.data_ptr(), ws.numel(), mm._row_ptr.data_ptr(), mm._ent.data_ptr(), mm._w.data_ptr(),
                mm.n_chunks, mm.nnz, split, n_split, cws, cb, st), "rarc_khop_chunks")))
            entry["neighbourhood_4096"] = step(f"{name}-{case}-list", 300, lambda: windows(
                torch, lambda: g.neighbourhood(sd, hops=hops, max_vertices=4096, as_device=True)))
            entry["neighbourhood_chunks_top10"] = step(f"{name}-{case}-chunks", 300, lambda: windows(
                torch, lambda: g.neighbourhood_chunks(mm, sd, hops=hops, top_k=10, as_device=True)))
            hc = g.neighbourhood(sd, hops=hops, max_vertices=1)[3]
            entry["mean_vertices_per_hop"] = [round(float(x), 1) for x in hc.mean(axis=0)]
            secs, how = step(f"{name}-{case}-host", 900, lambda: host_route(n, edges_host, seeds, hops, 4096))
            entry["host"] = {"seconds": round(secs, 4), "how": how}
            res["cases"][case] = entry
            print(json.dumps({name: {case: entry}}), flush=True)
        if nq == 256:                                               # a PageRank step on the same graph, in the same run
            wd = torch.ones((nq, 5), dtype=torch.int32, device=g.device)
            ws = torch.empty(int(lib.rarc_ppr_workspace_bytes(n, m, nq)), dtype=torch.uint8, device=g.device)

            def ppr_steps():
                B.check(lib.rarc_ppr_seed(gb.data_ptr(), gb.numel(), n, m, sd.data_ptr(), wd.data_ptr(), nq, 5, ws.data_ptr(), ws.numel(), st),
                        "rarc_ppr_seed")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cur = 0
                for _ in range(PPR_STEPS):
                    B.check(lib.rarc_ppr_step(gb.data_ptr(), gb.numel(), n, m, nq, 55706, 0, cur, ws.data_ptr(), ws.numel(), None, st),
                            "rarc_ppr_step")
                    cur ^= 1
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            ms = step(f"{name}-ppr-steps", 300, lambda: [ppr_steps() for _ in range(5)][2:])
            res["ppr_step_ms_256"] = round(statistics.median(ms) / PPR_STEPS, 4)
            slowest = max(max(res["cases"][f"hops{h}-nq256"]["step_ms"]) for h in (2, 3))
            res["slowest_khop_step_ms_256"] = slowest
            res["khop_step_faster_than_ppr_step"] = bool(slowest < res["ppr_step_ms_256"])
            del ws
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--graphs", default="planted_partition,duplicate_groups")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as KH
    from rag_arc_amd.encapsulation.database.graph_db import pagerank as PG
    from rag_arc_amd.encapsulation.database.graph_db import passages as PS
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    peak = step("peak", 120, lambda: stream_read_peak(torch, lib, B, dev))
    res = {"device": torch.cuda.get_device_name(0), "peak_measured_GBps": peak, "limits": KH.limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; "
                     "a step: device events around one launch group, the median of the last 3 of 5 seeded runs"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "planted_partition" in a.graphs:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_graph(torch, lib, B, PG, PS, KH, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges,
                                               peak, a)
        del edges
        torch.cuda.empty_cache()
        save()
    if "duplicate_groups" in a.graphs:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        pairs = pairs[:found].contiguous()
        del x
        res["duplicate_groups"] = bench_graph(torch, lib, B, PG, PS, KH, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy(), peak, a)
        save()


if __name__ == "__main__":
    main()
