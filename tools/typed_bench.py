#!/usr/bin/env python3
"""Typed traversal on the GPU, timed next to the untyped traversal of the same run and next to the route it replaces (DESIGN
4.13l).  GPU only, one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the process —
nothing more is started behind a hang).

The two graphs of tools/khop_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex, and
the duplicate-group graph of --rows x 768 Gaussian rows), every edge given one of four types uniformly at random.  256 queries of
five random seeds, once with random non-empty filters and once sharing one filter ({0, 1}).  Per graph and filter set, hops = 2:
  * rarc_graph_types: host clock around the call (it ends in a wait for the stream), median and range of five;
  * each step, typed and untyped, of the same seeds in the same run: device events around one launch group, median and range
    of the last three of five seeded runs;
  * EntityGraph.neighbourhood(max_vertices=4096) and .neighbourhood_edges() with relation_types= next to their untyped twins,
    answers left on the device: ms per call by the method of tools/ppr_bench.py;
  * the route the typed call replaces, one timed run: group the queries by filter, filter the pair list on the host, build one
    EntityGraph per distinct filter and run the untyped neighbourhood(max_vertices=4096) per group.

    python3 tools/typed_bench.py --out profiles/typed_bench.json
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

N_TYPES, NQ, HOPS = 4, 256, 2


def spread(xs):
    return {"ms": round(statistics.median(xs), 4), "range_ms": [round(min(xs), 4), round(max(xs), 4)]}


def bench_graph(torch, lib, B, PG, KH, name, n, pairs_dev, edges_host):
    rng = np.random.default_rng(17)
    types = rng.integers(0, N_TYPES, size=len(edges_host))
    g = PG.EntityGraph(n, pairs_dev, types=types)
    m = g.m
    res = {"vertices": n, "edges": m, "types": N_TYPES, "queries": NQ, "hops": HOPS, "cases": {}}
    st = torch.cuda.current_stream(g.device).cuda_stream
    gb = g._graph

    def build_types():
        out = []
        for _ in range(5):
            g._typed_adj = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            KH.typed_adjacency(g)
            out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)
    res["graph_types"] = step(f"{name}-graph-types", 120, build_types)
    ta = KH.typed_adjacency(g)
    seeds = rng.integers(0, n, (NQ, 5))
    sd = torch.from_numpy(seeds).to(g.device)
    filter_sets = {"random_filters": rng.integers(1, 1 << N_TYPES, size=NQ).astype(np.uint32), "one_filter": np.full(NQ, 0b0011, np.uint32)}
    for case, filters in filter_sets.items():
        fd = torch.from_numpy(filters.view(np.int32)).to(g.device)
        entry = {"distinct_filters": int(len(np.unique(filters)))}

        def seeded_steps(typed):
            """-> ms of each step, one event pair per step"""
            need = int(lib.rarc_khop_workspace_bytes(n, m, NQ, HOPS))
            if getattr(g, "_khop_ws", None) is None or g._khop_ws.numel() < need:
                g._khop_ws = torch.empty(need, dtype=torch.uint8, device=g.device)
            ws = g._khop_ws
            B.check(lib.rarc_khop_seed(n, m, sd.data_ptr(), NQ, 5, HOPS, ws.data_ptr(), ws.numel(), st), "rarc_khop_seed")
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(HOPS + 1)]
            ev[0].record()
            for hop in range(1, HOPS + 1):
                if typed:
                    B.check(lib.rarc_khop_step_typed(gb.data_ptr(), gb.numel(), ta.data_ptr(), ta.numel(), fd.data_ptr(), n, m, NQ, HOPS, hop,
                                                     ws.data_ptr(), ws.numel(), None, st), "rarc_khop_step_typed")
                else:
                    B.check(lib.rarc_khop_step(gb.data_ptr(), gb.numel(), n, m, NQ, HOPS, hop, ws.data_ptr(), ws.numel(), None, st), "rarc_khop_step")
                ev[hop].record()
            ev[HOPS].synchronize()
            return [ev[i].elapsed_time(ev[i + 1]) for i in range(HOPS)]
        for typed in (False, True):
            runs = step(f"{name}-{case}-steps-{typed}", 300, lambda: [seeded_steps(typed) for _ in range(5)][2:])
            entry["typed_step" if typed else "untyped_step"] = [spread([r[i] for r in runs]) for i in range(HOPS)]
        entry["typed_over_untyped_step"] = [round(t["ms"] / u["ms"], 3) for t, u in zip(entry["typed_step"], entry["untyped_step"])]
        for label, kw in (("untyped", {}), ("typed", {"relation_types": filters})):
            entry[f"neighbourhood_4096_{label}"] = step(f"{name}-{case}-list-{label}", 300, lambda: windows(
                torch, lambda: g.neighbourhood(sd, hops=HOPS, max_vertices=4096, as_device=True, **kw)))
            entry[f"neighbourhood_edges_{label}"] = step(f"{name}-{case}-edges-{label}", 300, lambda: windows(
                torch, lambda: g.neighbourhood_edges(sd, hops=HOPS, as_device=True, **kw)))

        def replaced_route():
            """one graph per distinct filter from host-filtered pairs, the untyped call per group -> (seconds, seconds in builds)"""
            torch.cuda.synchronize()
            t0, built = time.perf_counter(), 0.0
            for f in np.unique(filters):
                keep = ((np.uint32(1) << types.astype(np.uint32)) & f) != 0
                tb = time.perf_counter()
                sub = PG.EntityGraph(n, torch.from_numpy(edges_host[keep]).to(g.device))
                built += time.perf_counter() - tb
                sub.neighbourhood(sd[torch.from_numpy(np.flatnonzero(filters == f)).to(g.device)], hops=HOPS, max_vertices=4096, as_device=True)
                del sub
            torch.cuda.synchronize()
            return time.perf_counter() - t0, built
        secs, built = step(f"{name}-{case}-replaced", 600, replaced_route)
        entry["replaced_route"] = {"ms": round(secs * 1e3, 2), "of_which_graph_builds_ms": round(built * 1e3, 2),
                                   "how": "per distinct filter: numpy mask over the pair list, upload, EntityGraph, untyped neighbourhood(4096)"}
        hc = g.neighbourhood(sd, hops=HOPS, max_vertices=1, relation_types=filters)[3]
        entry["mean_vertices_per_hop_typed"] = [round(float(x), 1) for x in hc.mean(axis=0)]
        res["cases"][case] = entry
        print(json.dumps({name: {case: entry}}), flush=True)
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
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; "
                     "a step: device events around one launch group, median and range of the last 3 of 5 seeded runs; rarc_graph_types and "
                     "the replaced route: host clock"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "planted_partition" in a.graphs:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_graph(torch, lib, B, PG, KH, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges)
        del edges
        torch.cuda.empty_cache()
        save()
    if "duplicate_groups" in a.graphs:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        pairs = pairs[:found].contiguous()
        del x
        res["duplicate_groups"] = bench_graph(torch, lib, B, PG, KH, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy())
        save()


if __name__ == "__main__":
    main()
