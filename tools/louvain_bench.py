#!/usr/bin/env python3
"""Louvain communities on the GPU, timed next to what else the box has.  GPU only, one process; every step runs
under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

  1. entity_clusters on n x 768 Gaussian rows with planted near-duplicate groups (a tenth of the rows, groups of 2..60, noise
     0.02 per coordinate): the whole call, and its two parts timed on their own in the same process — the pairs
     (rarc_similar_pairs' launch loop, pairs left on the device) and the clustering of those pairs (labels copied to the host);
     beside them similar_pairs' own time (pairs sorted and copied to the host).
  2. the clustering alone on a synthetic planted-partition edge list: --vertices vertices in blocks of 20, each pair inside a
     block joined with probability 0.5 and 0.1 edges per vertex across blocks.
  3. networkx.community.louvain_communities on the host for the same edge lists (--networkx, where networkx is installed; an
     edge list beyond --networkx-max-edges is not given to it and the JSON says so), with its modularity beside this rule's.
Each GPU timing: `--warmup` unmeasured calls, then `--repeats` measured ones; the JSON carries every repeat (min / median / max).

    python3 tools/louvain_bench.py --rows 100000 --vertices 1000000 --networkx --out profiles/louvain_bench.json
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


def step(name, limit_s, fn):
    """fn() under a time limit of its own; an overrun or an error ends the process."""
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(int(limit_s))
    try:
        return fn()
    except StepTimeout:
        print(f"louvain_bench: step '{name}' exceeded {limit_s} s: stopping", file=sys.stderr, flush=True)
        os._exit(124)
    finally:
        signal.alarm(0)


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"s": out, "min_s": min(out), "median_s": statistics.median(out), "max_s": max(out)}


def make_rows(torch, n, d, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)
    rng = np.random.default_rng(seed)
    sizes, left = [], n // 10
    while left >= 2:
        s = int(min(left, rng.integers(2, 61)))
        sizes.append(s)
        left -= s
    rows = torch.randperm(n, generator=g, device="cuda")[:sum(sizes)]
    centre = torch.repeat_interleave(rows[torch.tensor(np.cumsum([0] + sizes[:-1]), device="cuda")],
                                     torch.tensor(sizes, device="cuda"))
    x[rows] = x[centre] + 0.02 * torch.randn((len(rows), d), generator=g, device="cuda")
    return x, sizes


def planted_edges(n, block, p_in, across_per_vertex, seed):
    rng = np.random.default_rng(seed)
    iu = np.stack(np.triu_indices(block, 1), axis=1)
    n_blocks = n // block
    keep = rng.random((n_blocks, len(iu))) < p_in
    b, e = np.nonzero(keep)
    inside = iu[e] + (b * block)[:, None]
    across = rng.integers(0, n, (int(across_per_vertex * n), 2))
    across = across[across[:, 0] // block != across[:, 1] // block]
    edges = np.concatenate([inside, across]).astype(np.int64)
    edges = np.unique(np.stack([edges.min(axis=1), edges.max(axis=1)], axis=1), axis=0)
    return edges


def modularity(n, edges, labels):
    k = np.bincount(edges.ravel(), minlength=n).astype(np.float64)
    m2 = k.sum()
    inside = 2.0 * np.count_nonzero(labels[edges[:, 0]] == labels[edges[:, 1]])
    tot = np.bincount(labels, weights=k, minlength=n)
    return float(inside / m2 - np.sum(tot * tot) / (m2 * m2))


def networkx_run(n, edges, limit_s):
    import networkx as nx

    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(edges.tolist())
    t0 = time.perf_counter()
    parts = step("networkx", limit_s, lambda: nx.community.louvain_communities(G, seed=0))
    dt = time.perf_counter() - t0
    labels = np.empty(n, np.int64)
    for p in parts:
        p = sorted(p)
        labels[p] = p[0]
    return {"seconds": dt, "communities": len(parts), "modularity": modularity(n, edges, labels), "version": nx.__version__}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--networkx", action="store_true")
    ap.add_argument("--networkx-limit", type=int, default=900)
    ap.add_argument("--networkx-max-edges", type=int, default=1000000, help="larger edge lists are not given to networkx")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database.graph_db import communities as C
    from rag_arc_amd.encapsulation.database.graph_db import entity_clusters, louvain_communities, similar_pairs
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "repeats": a.repeats, "bucket_limits": C.bucket_limits()}

    # 1. entity_clusters and its parts
    x, sizes = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
    pairs, _, found = S._pairs_on_device(lib, x, 0.95, dev)
    labels = entity_clusters(x, as_labels=True)
    edges = pairs[:found].cpu().numpy()
    ent = {"rows": a.rows, "dim": a.dim, "planted_groups": len(sizes), "planted_rows": int(sum(sizes)), "pairs": int(found),
           "communities_of_2_or_more": int(np.sum(np.bincount(labels, minlength=a.rows) >= 2)),
           "modularity": modularity(a.rows, edges, labels)}
    ent["entity_clusters"] = step("entity_clusters", 300, lambda: timed(torch, lambda: entity_clusters(x, as_labels=True), a.warmup, a.repeats))
    ent["pairs_on_device"] = step("pairs", 300, lambda: timed(torch, lambda: S._pairs_on_device(lib, x, 0.95, dev), a.warmup, a.repeats))
    ent["clustering"] = step("clustering", 300, lambda: timed(
        torch, lambda: C._cluster_on_device(lib, pairs, a.rows, found, 10, 10, dev).cpu(), a.warmup, a.repeats))
    ent["similar_pairs"] = step("similar_pairs", 300, lambda: timed(torch, lambda: similar_pairs(x, 0.95, as_arrays=True), a.warmup, a.repeats))
    if a.networkx:
        ent["networkx"] = networkx_run(a.rows, edges, a.networkx_limit)
    res["entity_clusters"] = ent
    print(json.dumps({k: (v if not isinstance(v, dict) or "median_s" not in v else round(v["median_s"], 5)) for k, v in ent.items()}),
          flush=True)
    del x, pairs

    # 2. the clustering alone
    n = a.vertices
    edges = step("edges", 300, lambda: planted_edges(n, 20, 0.5, 0.1, 2))
    dpairs = torch.from_numpy(edges).to(dev)
    labels = louvain_communities(n, dpairs)
    syn = {"vertices": n, "edges": int(len(edges)), "block": 20, "communities": int(len(np.unique(labels))),
           "modularity": modularity(n, edges, labels)}
    syn["clustering"] = step("clustering-1m", 400, lambda: timed(
        torch, lambda: C._cluster_on_device(lib, dpairs, n, len(edges), 10, 10, dev).cpu(), a.warmup, a.repeats))
    if a.networkx:
        syn["networkx"] = (networkx_run(n, edges, a.networkx_limit) if len(edges) <= a.networkx_max_edges else
                           f"not measured: {len(edges)} edges exceed --networkx-max-edges {a.networkx_max_edges}")
    res["planted_partition"] = syn
    print(json.dumps({k: (v if not isinstance(v, dict) or "median_s" not in v else round(v["median_s"], 5)) for k, v in syn.items()}),
          flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
