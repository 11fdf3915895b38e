#!/usr/bin/env python3
"""Typed personalized PageRank on the GPU, timed next to the untyped PageRank of the same run and next to the route it replaces
(DESIGN 4.13m).  GPU only, one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the
process — nothing more is started behind a hang).

The two graphs of tools/typed_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex, and
the duplicate-group graph of --rows x 768 Gaussian rows), every edge given one of four types uniformly at random; five random
seeds a query, --iterations steps, top_k --top-k.  Per graph, by the method of tools/ppr_bench.py:
  * rarc_graph_types_weighted next to rarc_graph_types: host clock around the call (each ends in a wait for the stream), median
    and range of five;
  * at B = 1 and B = 256, with random non-empty filters and with one shared filter ({0, 1}): a typed step and an untyped step
    (the iterations between two device events after a fresh seed, median of the last three of five, divided by the iterations),
    the bytes a typed step moves by count — (2 m + 4 n) state rows of 8 B bytes, 12 bytes a slot for neighbour, mask and
    weight against the untyped 8, the row pointers — and the typed call next to the untyped call, answers left on the device;
  * the route the typed call replaces at B = 256, one timed run each for 15 random filters and for one shared filter: group the
    queries by filter, filter the pair list on the host, build one EntityGraph per distinct filter and run the untyped call
    per group.

    python3 tools/typed_ppr_bench.py --out profiles/typed_ppr_bench.json
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
from typed_bench import spread  # noqa: E402

N_TYPES, DAMPING_Q16 = 4, 55706


def bench_graph(torch, lib, B, PG, KH, name, n, pairs_dev, edges_host, a):
    rng = np.random.default_rng(17)
    types = rng.integers(0, N_TYPES, size=len(edges_host))
    g = PG.EntityGraph(n, pairs_dev, types=types)
    m = g.m
    res = {"vertices": n, "edges": m, "types": N_TYPES, "iterations": a.iterations, "top_k": a.top_k, "batches": {}}
    st = torch.cuda.current_stream(g.device).cuda_stream
    gb = g._graph

    def build(weighted):
        out = []
        for _ in range(5):
            g._typed_adj = g._typed_adj_weighted = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            KH.typed_adjacency(g, weighted=weighted)
            out.append((time.perf_counter() - t0) * 1e3)
        return spread(out)
    res["graph_types"] = step(f"{name}-graph-types", 120, lambda: build(False))
    res["graph_types_weighted"] = step(f"{name}-graph-types-weighted", 120, lambda: build(True))
    ta = KH.typed_adjacency(g, weighted=True)
    for nq in (1, 256):
        seeds = rng.integers(0, n, (nq, 5))
        sd = torch.from_numpy(seeds).to(g.device)
        wd = torch.ones((nq, 5), dtype=torch.int32, device=g.device)
        filter_sets = {"random_filters": rng.integers(1, 1 << N_TYPES, size=nq).astype(np.uint32), "one_filter": np.full(nq, 0b0011, np.uint32)}
        entry = {}
        for case, filters in filter_sets.items():
            fd = torch.from_numpy(filters.view(np.int32)).to(g.device)
            sub = {"distinct_filters": int(len(np.unique(filters)))}
            for label, kw in (("untyped", {}), ("typed", {"relation_types": filters})):
                sub[f"call_{label}"] = step(f"{name}-{nq}-{case}-call-{label}", 300, lambda: windows(
                    torch, lambda: g.personalized_pagerank(sd, max_iterations=a.iterations, top_k=a.top_k, as_device=True, **kw)))
            ws = g._ws

            def seeded_steps(typed):
                """a fresh seed, then the iterations between two events -> ms"""
                if typed:
                    B.check(lib.rarc_ppr_seed_typed(gb.data_ptr(), gb.numel(), ta.data_ptr(), ta.numel(), fd.data_ptr(), n, m, sd.data_ptr(),
                                                    wd.data_ptr(), nq, 5, ws.data_ptr(), ws.numel(), st), "rarc_ppr_seed_typed")
                else:
                    B.check(lib.rarc_ppr_seed(gb.data_ptr(), gb.numel(), n, m, sd.data_ptr(), wd.data_ptr(), nq, 5, ws.data_ptr(), ws.numel(), st),
                            "rarc_ppr_seed")
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                cur = 0
                for _ in range(a.iterations):
                    if typed:
                        B.check(lib.rarc_ppr_step_typed(gb.data_ptr(), gb.numel(), ta.data_ptr(), ta.numel(), fd.data_ptr(), n, m, nq, DAMPING_Q16,
                                                        0, cur, ws.data_ptr(), ws.numel(), None, st), "rarc_ppr_step_typed")
                    else:
                        B.check(lib.rarc_ppr_step(gb.data_ptr(), gb.numel(), n, m, nq, DAMPING_Q16, 0, cur, ws.data_ptr(), ws.numel(), None, st),
                                "rarc_ppr_step")
                    cur ^= 1
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)
            for typed in (False, True):
                ms = step(f"{name}-{nq}-{case}-steps-{typed}", 300, lambda: [seeded_steps(typed) for _ in range(5)][2:])
                sub["typed_step" if typed else "untyped_step"] = spread([x / a.iterations for x in ms])
            sub["typed_over_untyped_step"] = round(sub["typed_step"]["ms"] / sub["untyped_step"]["ms"], 3)
            state = (2 * m + 4 * n) * nq * 8
            sub["counted_bytes"] = {"untyped": state + 2 * m * 8 + n * 12, "typed": state + 2 * m * 12 + n * 8}
            sub["typed_over_untyped_bytes"] = round(sub["counted_bytes"]["typed"] / sub["counted_bytes"]["untyped"], 3)
            entry[case] = sub
        res["batches"][str(nq)] = entry
        print(json.dumps({name: {str(nq): entry}}), flush=True)

    # the route replaced, B = 256
    nq = 256
    seeds = rng.integers(0, n, (nq, 5))
    sd = torch.from_numpy(seeds).to(g.device)
    routes = {"15_random_filters": rng.integers(1, 1 << N_TYPES, size=nq).astype(np.uint32), "one_filter": np.full(nq, 0b0011, np.uint32)}
    res["replaced_route"] = {}
    for case, filters in routes.items():
        def replaced_route():
            """one graph per distinct filter from host-filtered pairs, the untyped call per group -> (seconds, seconds in builds)"""
            torch.cuda.synchronize()
            t0, built = time.perf_counter(), 0.0
            for f in np.unique(filters):
                keep = ((np.uint32(1) << types.astype(np.uint32)) & f) != 0
                tb = time.perf_counter()
                sub = PG.EntityGraph(n, torch.from_numpy(edges_host[keep]).to(g.device))
                built += time.perf_counter() - tb
                sub.personalized_pagerank(sd[torch.from_numpy(np.flatnonzero(filters == f)).to(g.device)], max_iterations=a.iterations,
                                          top_k=a.top_k, as_device=True)
                del sub
            torch.cuda.synchronize()
            return time.perf_counter() - t0, built
        secs, built = step(f"{name}-{case}-replaced", 600, replaced_route)
        typed_call = step(f"{name}-{case}-typed-call", 300, lambda: windows(
            torch, lambda: g.personalized_pagerank(sd, max_iterations=a.iterations, top_k=a.top_k, as_device=True, relation_types=filters)))
        res["replaced_route"][case] = {"distinct_filters": int(len(np.unique(filters))), "ms": round(secs * 1e3, 2),
                                       "of_which_graph_builds_ms": round(built * 1e3, 2), "typed_call": typed_call,
                                       "how": "per distinct filter: numpy mask over the pair list, upload, EntityGraph, untyped "
                                              "personalized_pagerank(top_k) of its queries"}
    print(json.dumps({name: {"replaced_route": res["replaced_route"]}}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--top-k", type=int, default=10)
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
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; a step: "
                     "the iterations between two device events after a fresh seed, median and range of the last 3 of 5 runs, per iteration; "
                     "rarc_graph_types[_weighted] and the replaced route: host clock"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "planted_partition" in a.graphs:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_graph(torch, lib, B, PG, KH, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges, a)
        del edges
        torch.cuda.empty_cache()
        save()
    if "duplicate_groups" in a.graphs:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        pairs = pairs[:found].contiguous()
        del x
        res["duplicate_groups"] = bench_graph(torch, lib, B, PG, KH, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy(), a)
        save()


if __name__ == "__main__":
    main()
