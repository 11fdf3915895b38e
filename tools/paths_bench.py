#!/usr/bin/env python3
"""Connecting paths on the GPU, timed next to the host route they replace.  GPU only, one process; every step runs
under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

The two graphs of tools/khop_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex, and
the duplicate-group graph of --rows x 768 Gaussian rows), each with its own pair list as the relation table.  Per graph 256
one-vertex sources and 256 pairs over them, max_length 4: source 2i is a random vertex, source 2i + 1 the farthest vertex a 4-hop
neighbourhood of it lists, and the pairs are (2i, 2i + 1) and (2i + 1, 2i), so that most pairs have paths.
  * rarc_khop_paths alone on the state a traversal left, between two events, the median of five; the same for
    rarc_khop_path_edges on the path state it wrote;
  * EntityGraph.shortest_paths, answers left on the device — traversal, distances, mark, the vertex list, the relation rows and
    the gather of their ends: ms per call by the method of tools/ppr_bench.py (the `method` string records it);
  * the host route it replaces, in the same run: from the dense levels neighbourhood() left on the device, the copy to the host,
    then per pair the mask hop_A + hop_B == d, a lexsort of the vertices on the paths by (position, vertex), and the mask of the
    pair list (ends at consecutive positions) with a stable sort by level; one timed run;
  * every pair's distance, and the vertex and relation lists of one pair with the longest paths found, are compared between the
    two routes before any time is reported.

    python3 tools/paths_bench.py --out profiles/paths_bench.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from khop_edges_bench import between_events  # noqa: E402
from louvain_bench import make_rows, planted_edges, step  # noqa: E402
from ppr_bench import windows  # noqa: E402

MAX_EDGES, MAX_VERTICES, LENGTH, SOURCES = 16384, 4096, 4, 256


def host_route(levels_dev, pairs, table, max_vertices, max_edges):
    """device uint8 [ns][n] levels -> (seconds, distances, per pair (vertices, positions, rows, levels), cut at the caps)"""
    t0 = time.perf_counter()
    lv = levels_dev.cpu().numpy()
    a, b = table[:, 0], table[:, 1]
    dist, out = [], []
    for ia, ib in pairs:
        ha, hb = lv[ia].astype(np.int16), lv[ib].astype(np.int16)                 # 255 = "not within max_length": any sum with it is > 8
        both = ha + hb
        d = int(both.min())
        if d > LENGTH:
            dist.append(-1)
            out.append(None)
            continue
        pos = np.where(both == d, ha, 255)
        on = np.flatnonzero(pos != 255)
        order = on[np.lexsort((on, pos[on]))][:max_vertices]
        pa, pb = pos[a], pos[b]
        rows = np.flatnonzero((pa != 255) & (pb != 255) & (np.abs(pa - pb) == 1))
        level = np.maximum(pa[rows], pb[rows])
        keep = np.argsort(level, kind="stable")[:max_edges]
        dist.append(d)
        out.append((order, pos[order], rows[keep], level[keep]))
    return time.perf_counter() - t0, np.asarray(dist, np.int32), out


def bench_graph(torch, lib, B, PG, KH, name, n, pairs_dev, pairs_host):
    g = PG.EntityGraph(n, pairs_dev)
    m = g.m
    rel = KH._own_relations(g)
    rng = np.random.default_rng(11)
    st = torch.cuda.current_stream(g.device).cuda_stream
    first = rng.integers(0, n, SOURCES // 2)
    ids, _, counts, _ = g.neighbourhood([[int(v)] for v in first], hops=LENGTH, max_vertices=MAX_VERTICES)
    far = ids[np.arange(len(first)), counts - 1]                                  # the last listed vertex: one at the farthest hop listed
    sources = np.stack([first, far], axis=1).reshape(-1, 1).astype(np.int64)
    pairs = np.asarray([(2 * i + s, 2 * i + 1 - s) for i in range(SOURCES // 2) for s in (0, 1)], np.int32)
    sd, pd = torch.from_numpy(sources).to(g.device), torch.from_numpy(pairs).to(g.device)
    ns, npairs = len(sources), len(pairs)
    entry = {"vertices": n, "edges": m, "relations": rel.r, "sources": ns, "pairs": npairs, "max_length": LENGTH, "max_vertices": MAX_VERTICES,
             "max_edges": MAX_EDGES}
    ws, wb = step(f"{name}-traverse", 120, lambda: KH.traverse(g, sd, LENGTH))
    pws = torch.empty(int(lib.rarc_khop_workspace_bytes(n, m, npairs, LENGTH)), dtype=torch.uint8, device=g.device)
    dist = torch.empty(npairs, dtype=torch.int32, device=g.device)
    entry["paths_ms"] = step(f"{name}-paths-alone", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_khop_paths(
        n, m, ns, npairs, LENGTH, ws, wb, pd.data_ptr(), pws.data_ptr(), pws.numel(), dist.data_ptr(), st), "rarc_khop_paths")))
    ews = torch.empty(int(lib.rarc_khop_edges_workspace_bytes(rel.r, npairs, LENGTH)), dtype=torch.uint8, device=g.device)
    eids = torch.empty((npairs, MAX_EDGES), dtype=torch.int64, device=g.device)
    elv = torch.empty((npairs, MAX_EDGES), dtype=torch.int32, device=g.device)
    cnt = torch.empty(npairs, dtype=torch.int32, device=g.device)
    lc = torch.empty((npairs, LENGTH + 1), dtype=torch.int32, device=g.device)
    entry["path_edges_ms"] = step(f"{name}-path-edges-alone", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_khop_path_edges(
        n, m, npairs, LENGTH, pws.data_ptr(), pws.numel(), rel._pairs.data_ptr(), rel.r, MAX_EDGES, ews.data_ptr(), ews.numel(), eids.data_ptr(),
        elv.data_ptr(), cnt.data_ptr(), lc.data_ptr(), st), "rarc_khop_path_edges")))
    entry["state_bytes"] = {"traversal": int(lib.rarc_khop_workspace_bytes(n, m, ns, LENGTH)), "paths": pws.numel(), "edge_counts": ews.numel()}
    del pws, ews, eids, elv
    entry["traverse"] = step(f"{name}-traverse-call", 300, lambda: windows(torch, lambda: KH.traverse(g, sd, LENGTH)))
    entry["shortest_paths"] = step(f"{name}-call", 300, lambda: windows(torch, lambda: g.shortest_paths(
        sd, pd, max_length=LENGTH, max_vertices=MAX_VERTICES, max_edges=MAX_EDGES, as_device=True)))
    got = g.shortest_paths(sd, pd, max_length=LENGTH, max_vertices=MAX_VERTICES, max_edges=MAX_EDGES)
    entry["distances"] = {str(d): int((got.distances == d).sum()) for d in range(-1, LENGTH + 1)}
    entry["mean_vertices_per_position"] = [round(float(x), 1) for x in got.position_counts.mean(axis=0)]
    entry["mean_relations_per_level"] = [round(float(x), 1) for x in got.edge_level_counts.mean(axis=0)]
    entry["neighbourhood_dense"] = step(f"{name}-dense", 300, lambda: windows(torch, lambda: g.neighbourhood(sd, hops=LENGTH, as_device=True)))
    dense = g.neighbourhood(sd, hops=LENGTH, as_device=True)
    torch.cuda.synchronize()
    secs, hd, lists = step(f"{name}-host", 900, lambda: host_route(dense, pairs.tolist(), pairs_host, MAX_VERTICES, MAX_EDGES))
    del dense
    assert np.array_equal(hd, got.distances)
    p = int(np.argmax(got.distances))                                             # a pair with the longest paths found
    vc, ec = int(got.vertex_counts[p]), int(got.edge_counts[p])
    assert vc == len(lists[p][0]) and np.array_equal(got.vertex_ids[p, :vc], lists[p][0]) and np.array_equal(got.vertex_positions[p, :vc], lists[p][1])
    assert ec == len(lists[p][2]) and np.array_equal(got.edge_ids[p, :ec], lists[p][2]) and np.array_equal(got.edge_levels[p, :ec], lists[p][3])
    entry["host"] = {"seconds": round(secs, 4), "how": "dense levels device -> host, then per pair numpy: hop_A + hop_B == d, lexsort of the "
                                                       "on-path vertices by (position, vertex), mask of the pair list by consecutive positions, "
                                                       "stable argsort by level"}
    entry["call_faster_than_host_route"] = bool(entry["shortest_paths"]["ms"] * 1e-3 < secs)
    print(json.dumps({name: entry}), flush=True)
    return entry


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
    res = {"device": torch.cuda.get_device_name(0), "limits": KH.paths_limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s (all "
                     "windows listed); an entry alone: device events around one launch group, the median of 5; the host route: one timed run"}

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
