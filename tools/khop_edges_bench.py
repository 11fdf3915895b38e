#!/usr/bin/env python3
"""k-hop subgraphs on the GPU, timed next to the host route they replace and next to the vertex list.  GPU only,
one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started
behind a hang).

The two graphs of tools/khop_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex, and
the duplicate-group graph of --rows x 768 Gaussian rows), each with its own pair list as the relation table.  Per graph, hops
(2 and 3) and batch (1 and 256 queries of five random seeds), max_edges 16384:
  * rarc_khop_edges alone on the state a traversal left, between two events, the median of five; the same for its count and
    scan passes alone (null list outputs) and for rarc_khop_list (max_vertices 4096) on the same state;
  * EntityGraph.neighbourhood_edges, answers left on the device — traversal, the three passes and the gather of the ends:
    ms per call by the method of tools/ppr_bench.py (the `method` string records it);
  * the host route it replaces, in the same run: from the dense levels neighbourhood() left on the device, the copy to the host,
    then per query the mask of the pair list (both ends within hops) and the stable sort of the surviving rows by level; one
    timed run per case, and beside it the neighbourhood() call that produces those levels (it is not part of the route's time);
  * the first query's list of both routes is compared before any time is reported.

    python3 tools/khop_edges_bench.py --out profiles/khop_edges_bench.json
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

MAX_EDGES, MAX_VERTICES = 16384, 4096


def host_route(levels_dev, pairs, max_edges):
    """device uint8 [B][n] levels -> (seconds, per query the (rows, levels) of its list, cut at max_edges)"""
    t0 = time.perf_counter()
    lv = levels_dev.cpu().numpy()
    a, b = pairs[:, 0], pairs[:, 1]
    out = []
    for q in range(lv.shape[0]):
        level = np.maximum(lv[q][a], lv[q][b])                     # 255 = "not within hops" is the largest value
        rows = np.flatnonzero(level != 255)
        order = rows[np.argsort(level[rows], kind="stable")][:max_edges]
        out.append((order, level[order]))
    return time.perf_counter() - t0, out


def between_events(torch, fn):
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def bench_graph(torch, lib, B, PG, KH, name, n, pairs_dev, pairs_host):
    g = PG.EntityGraph(n, pairs_dev)
    m = g.m
    rel = KH._own_relations(g)
    rng = np.random.default_rng(11)
    res = {"vertices": n, "edges": m, "relations": rel.r, "cases": {}}
    st = torch.cuda.current_stream(g.device).cuda_stream
    for nq in (1, 256):
        seeds = rng.integers(0, n, (nq, 5))
        sd = torch.from_numpy(seeds).to(g.device)
        for hops in (2, 3):
            case = f"hops{hops}-nq{nq}"
            entry = {"hops": hops, "queries": nq, "max_edges": MAX_EDGES}
            ws, wb = step(f"{name}-{case}-traverse", 120, lambda: KH.traverse(g, sd, hops))
            ews = torch.empty(int(lib.rarc_khop_edges_workspace_bytes(rel.r, nq, hops)), dtype=torch.uint8, device=g.device)
            ids = torch.empty((nq, MAX_EDGES), dtype=torch.int64, device=g.device)
            lv = torch.empty((nq, MAX_EDGES), dtype=torch.int32, device=g.device)
            cnt = torch.empty(nq, dtype=torch.int32, device=g.device)
            lc = torch.empty((nq, hops + 1), dtype=torch.int32, device=g.device)
            vids = torch.empty((nq, MAX_VERTICES), dtype=torch.int64, device=g.device)
            vhp = torch.empty((nq, MAX_VERTICES), dtype=torch.int32, device=g.device)

            def edges(listed):
                p = (lambda x: x.data_ptr()) if listed else (lambda x: None)
                B.check(lib.rarc_khop_edges(n, m, nq, hops, ws, wb, rel._pairs.data_ptr(), rel.r, MAX_EDGES, ews.data_ptr(), ews.numel(), p(ids),
                                            p(lv), p(cnt), lc.data_ptr(), st), "rarc_khop_edges")
            entry["edges_ms"] = step(f"{name}-{case}-edges-alone", 120, lambda: between_events(torch, lambda: edges(True)))
            entry["edges_count_scan_ms"] = step(f"{name}-{case}-edges-counts", 120, lambda: between_events(torch, lambda: edges(False)))
            entry["list_ms"] = step(f"{name}-{case}-list-alone", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_khop_list(
                n, m, nq, hops, MAX_VERTICES, ws, wb, vids.data_ptr(), vhp.data_ptr(), cnt.data_ptr(), st), "rarc_khop_list")))
            entry["edge_workspace_bytes"] = ews.numel()
            entry["neighbourhood_edges"] = step(f"{name}-{case}-call", 300, lambda: windows(
                torch, lambda: g.neighbourhood_edges(sd, hops=hops, max_edges=MAX_EDGES, as_device=True)))
            got = g.neighbourhood_edges(sd, hops=hops, max_edges=MAX_EDGES)
            entry["mean_relations_per_level"] = [round(float(x), 1) for x in got.edge_level_counts.mean(axis=0)]
            entry["queries_cut_by_max_edges"] = int((got.edge_level_counts.sum(axis=1) > MAX_EDGES).sum())
            entry["neighbourhood_dense"] = step(f"{name}-{case}-dense", 300, lambda: windows(
                torch, lambda: g.neighbourhood(sd, hops=hops, as_device=True)))
            dense = g.neighbourhood(sd, hops=hops, as_device=True)
            torch.cuda.synchronize()
            secs, lists = step(f"{name}-{case}-host", 900, lambda: host_route(dense, pairs_host, MAX_EDGES))
            del dense
            c = int(got.edge_counts[0])
            assert c == len(lists[0][0]) and np.array_equal(got.edge_ids[0, :c], lists[0][0]) and np.array_equal(got.edge_levels[0, :c], lists[0][1])
            entry["host"] = {"seconds": round(secs, 4), "how": "dense levels device -> host, then per query numpy: max of the two ends' levels, "
                                                               "flatnonzero, stable argsort by level"}
            entry["call_faster_than_host_route"] = bool(entry["neighbourhood_edges"]["ms"] * 1e-3 < secs)
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
    res = {"device": torch.cuda.get_device_name(0), "limits": KH.edges_limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; "
                     "an entry alone: device events around one launch group, the median of 5; the host route: one timed run"}

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
