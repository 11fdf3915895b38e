#!/usr/bin/env python3
"""Connected components on the GPU, timed next to the host route they replace, next to Louvain and next to a k-hop step (DESIGN
4.13j).  GPU only, one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the process —
nothing more is started behind a hang).

The two graphs of tools/khop_bench.py and tools/merge_bench.py (the planted-partition edge list of --vertices vertices, about 4.8
edges per vertex, and the duplicate-group graph of --rows x 768 Gaussian rows).  Per graph, in one run:
  * the rounds taken, and every round alone: after an init, each rarc_components_round between two events of its own (no word is
    read back in between: a round past the last changes nothing), the median and the range of the last three of five runs; the
    finish likewise;
  * EntityGraph.components() from scratch (the kept answer dropped before every call), the answer left on the device and copied
    to the host: ms per call by the method of tools/ppr_bench.py, every window listed;
  * the host route: scipy.sparse.csgraph.connected_components over the same pairs, the matrix build counted and not counted;
  * Louvain's clustering of the same pairs (rarc_graph_csr + sweeps + aggregate, communities._cluster_on_device), three runs;
  * one rarc_khop_step at 256 queries of five seeds, hops 2 (both steps), as tools/khop_bench.py times it: the yardstick for a
    round, which reads the same adjacency.

    python3 tools/components_bench.py --out profiles/components_bench.json

--trace runs nothing but three labellings of the planted-partition graph, for a kernel trace that tools/components_kstats.py
takes apart into the hook launches and the jump of every round:

    rocprofv3 --kernel-trace --output-format csv -d D -- python3 tools/components_bench.py --trace
    python3 tools/components_kstats.py D
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


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def host_route(n, edges):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components

    t0 = time.perf_counter()
    a = sp.coo_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr()
    t1 = time.perf_counter()
    n_c, labels = connected_components(a, directed=False)
    t2 = time.perf_counter()
    return {"seconds": round(t2 - t0, 4), "seconds_without_matrix_build": round(t2 - t1, 4), "components": int(n_c),
            "how": "scipy.sparse.csgraph.connected_components(csr, directed=False) over the same pairs"}, labels


def bench_graph(torch, lib, B, db, CM, CC, name, n, pairs_dev, edges_host):
    g = db.EntityGraph(n, pairs_dev)
    m = g.m
    st = torch.cuda.current_stream(g.device).cuda_stream
    gb = g._graph
    res = {"vertices": n, "edges": m}
    first = g.components()
    rounds = first.rounds
    res.update({"rounds": rounds, "round_bound": CC.round_bound(n), "components": first.n_components, "largest": list(first.largest),
                "isolated_vertices": int(n - np.count_nonzero(np.bincount(edges_host.ravel(), minlength=n)))})
    ws = torch.empty(int(lib.rarc_components_workspace_bytes(n, m)), dtype=torch.uint8, device=g.device)
    changed = torch.zeros(1, dtype=torch.int32, device=g.device)
    labels = torch.empty(n, dtype=torch.int64, device=g.device)
    dense = torch.empty(n, dtype=torch.int32, device=g.device)
    sizes = torch.empty(n, dtype=torch.int64, device=g.device)
    out3 = torch.empty(3, dtype=torch.int64, device=g.device)

    def one_run():
        """-> ms of each round and of the finish, one event pair each"""
        B.check(lib.rarc_components_init(n, m, ws.data_ptr(), ws.numel(), st), "rarc_components_init")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(rounds + 2)]
        ev[0].record()
        for r in range(rounds):
            B.check(lib.rarc_components_round(gb.data_ptr(), gb.numel(), n, m, ws.data_ptr(), ws.numel(), changed.data_ptr(), st),
                    "rarc_components_round")
            ev[r + 1].record()
        B.check(lib.rarc_components_finish(n, m, ws.data_ptr(), ws.numel(), labels.data_ptr(), dense.data_ptr(), sizes.data_ptr(), out3.data_ptr(),
                                           st), "rarc_components_finish")
        ev[rounds + 1].record()
        ev[rounds + 1].synchronize()
        assert int(changed.item()) == 0 and out3.tolist() == [first.n_components, first.largest[1], first.largest[0]]
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(rounds + 1)]
    runs = step(f"{name}-rounds", 300, lambda: [one_run() for _ in range(5)][2:])
    res["round_ms"] = [spread([r[i] for r in runs]) for i in range(rounds)]
    res["finish_ms"] = spread([r[rounds] for r in runs])
    res["rounds_total_ms"] = spread([sum(r[:rounds]) for r in runs])
    # a round moves: the lists and row_ptr of the listed vertices, 2 m entries and their parents, n parents hooked, 2 n jumped
    moved = 2 * m * 8 + n * (4 + 16 + 4) + n * 12
    res["round_bytes"] = moved
    res["round_GBps"] = [round(moved / (x["median"] * 1e-3) / 1e9, 1) for x in res["round_ms"]]

    def fresh(as_device):
        g._components.clear()
        return g.components(as_device=as_device)
    res["components_device"] = step(f"{name}-components-device", 300, lambda: windows(torch, lambda: fresh(True)))
    res["components_host"] = step(f"{name}-components-host", 300, lambda: windows(torch, lambda: fresh(False)))
    host, host_labels = step(f"{name}-scipy", 900, lambda: host_route(n, edges_host))
    res["host"] = host
    assert host["components"] == first.n_components
    first_of = np.full(host["components"], n, np.int64)
    np.minimum.at(first_of, host_labels, np.arange(n))
    assert np.array_equal(first_of[host_labels], first.labels), "the labels differ from scipy's components"
    res["host_over_components_host"] = round(host["seconds"] * 1e3 / res["components_host"]["ms"], 1)

    def louvain():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        CM._cluster_on_device(lib, g._pairs, n, m, 10, 10, g.device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    res["louvain_ms"] = spread(step(f"{name}-louvain", 600, lambda: [louvain() for _ in range(4)][1:]))

    def labels_only():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        CC.labels_on_device(lib, g._pairs, n, m, g.device)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    res["labels_from_pairs_ms"] = spread(step(f"{name}-labels", 300, lambda: [labels_only() for _ in range(4)][1:]))

    nq, hops = 256, 2
    sd = torch.from_numpy(np.random.default_rng(11).integers(0, n, (nq, 5))).to(g.device)
    kws = torch.empty(int(lib.rarc_khop_workspace_bytes(n, m, nq, hops)), dtype=torch.uint8, device=g.device)

    def khop_steps():
        B.check(lib.rarc_khop_seed(n, m, sd.data_ptr(), nq, 5, hops, kws.data_ptr(), kws.numel(), st), "rarc_khop_seed")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(hops + 1)]
        ev[0].record()
        for hop in range(1, hops + 1):
            B.check(lib.rarc_khop_step(gb.data_ptr(), gb.numel(), n, m, nq, hops, hop, kws.data_ptr(), kws.numel(), None, st), "rarc_khop_step")
            ev[hop].record()
        ev[hops].synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(hops)]
    kruns = step(f"{name}-khop-steps", 300, lambda: [khop_steps() for _ in range(5)][2:])
    res["khop_step_ms_256"] = [spread([r[i] for r in kruns]) for i in range(hops)]
    slowest_step = max(x["median"] for x in res["khop_step_ms_256"])
    res["slowest_round_over_slowest_khop_step"] = round(max(x["median"] for x in res["round_ms"]) / slowest_step, 2)
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--graphs", default="planted_partition,duplicate_groups")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true", help="three labellings of the planted-partition graph and nothing else")
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database import graph_db as db
    from rag_arc_amd.encapsulation.database.graph_db import communities as CM
    from rag_arc_amd.encapsulation.database.graph_db import components as CC
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    if a.trace:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        g = db.EntityGraph(a.vertices, torch.from_numpy(edges).to(dev))
        for _ in range(3):
            g._components.clear()
            got = step("trace", 60, lambda: g.components(as_device=True))
            torch.cuda.synchronize()
        print(json.dumps({"vertices": g.n, "edges": g.m, "rounds": got.rounds, "components": got.n_components, "limits": CC.limits()}))
        return
    res = {"device": torch.cuda.get_device_name(0), "limits": CC.limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s, every "
                     "window listed; a round, the finish, a k-hop step: device events around one launch group, median / min / max of the "
                     "last 3 of 5 runs; Louvain and labels-from-pairs: host clock around one call, the last 3 of 4"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "planted_partition" in a.graphs:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_graph(torch, lib, B, db, CM, CC, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges)
        del edges
        torch.cuda.empty_cache()
        save()
    if "duplicate_groups" in a.graphs:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        pairs = pairs[:found].contiguous()
        del x
        res["duplicate_groups"] = bench_graph(torch, lib, B, db, CM, CC, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy())
        save()


if __name__ == "__main__":
    main()
