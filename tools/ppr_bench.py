#!/usr/bin/env python3
"""Personalized PageRank on the GPU, timed next to the host.  GPU only, one process; every step runs under its
own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

Two graphs, the ones tools/louvain_bench.py clusters: the planted-partition edge list (--vertices vertices in blocks of 20,
about 4.8 edges per vertex) and the duplicate-group graph of --rows x 768 Gaussian rows (the pairs rarc_similar_pairs finds at
0.95, left on the device).  Per graph and batch (1 and 256 queries of five random seeds): EntityGraph.personalized_pagerank
with 20 iterations and top_k 10, answers left on the device; ms per call by the method of DESIGN 4.10d — host clock around
calls ending in a synchronise, two warm-up calls, the median of three windows of >= 0.25 s.  Beside it:
  * the iteration alone (the same call with top_k and the seed subtracted out is not attempted: the step is timed directly,
    20 rarc_ppr_step launches between two events), and the bytes one iteration moves — (2 m + 4 n) state rows of 8 B bytes plus
    the adjacency — as a rate and as a fraction of this box's read stream (rarc_stream_read, bench.py's `peak_measured`);
  * the host: a float64 power iteration with scipy.sparse where scipy imports, else numpy (np.add.at over the edge list),
    the same 20 iterations on the same graph and seeds, one timed run per batch.

    python3 tools/ppr_bench.py --out profiles/ppr_bench.json
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


def windows(torch, fn, min_s=0.25, n_windows=3, warmup=2):
    """ms per call: the median of n_windows windows of at least min_s each, after `warmup` calls; all windows are returned"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        calls, t0 = 0, time.perf_counter()
        while True:
            fn()
            calls += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_s:
                break
        out.append(dt / calls * 1e3)
    return {"ms": round(statistics.median(out), 4), "windows_ms": [round(x, 4) for x in out]}


def stream_read_peak(torch, lib, B, dev):
    """GB/s of rarc_stream_read over 4 GiB: best of four passes after a warm-up pass (bench.py's peak_measured)"""
    nbytes = int(min(4 << 30, torch.cuda.mem_get_info(dev)[0] // 4))
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    sink = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        B.check(lib.rarc_stream_read(buf.data_ptr(), nbytes, sink.data_ptr(), st), "rarc_stream_read")
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(nbytes / (min(ms[1:]) * 1e-3) / 1e9, 1)


def host_power_iteration(n, edges, seeds, damping, iterations):
    """float64 [n][B] power iteration on the host -> (seconds, what ran)"""
    src = np.concatenate([edges[:, 0], edges[:, 1]])
    dst = np.concatenate([edges[:, 1], edges[:, 0]])
    deg = np.bincount(src, minlength=n).astype(np.float64)
    t = np.zeros((n, len(seeds)))
    for q, s in enumerate(seeds):
        np.add.at(t[:, q], s, 1.0 / len(s))
    inv = np.where(deg > 0, 1.0 / np.maximum(deg, 1.0), 0.0)[:, None]
    lone = (deg == 0)[:, None]
    try:
        import scipy.sparse as sp

        A = sp.csr_matrix((np.ones(len(src)), (dst, src)), shape=(n, n))
        how = "scipy.sparse csr @ dense, float64"
        flow = lambda c: A @ c                                     # noqa: E731
    except ImportError:
        how = "numpy np.add.at over the edge list, float64"

        def flow(c):
            out = np.zeros_like(c)
            np.add.at(out, dst, c[src])
            return out
    t0 = time.perf_counter()
    p = t.copy()
    for _ in range(iterations):
        p = (1.0 - damping) * t + damping * (flow(p * inv) + np.where(lone, p, 0.0))
    return time.perf_counter() - t0, how, p


def bench_graph(torch, lib, B, PG, name, n, pairs_dev, edges_host, peak, a):
    g = PG.EntityGraph(n, pairs_dev)
    m = g.m
    rng = np.random.default_rng(11)
    res = {"vertices": n, "edges": m, "iterations": a.iterations, "top_k": a.top_k, "batches": {}}
    for nq in (1, 256):
        seeds = rng.integers(0, n, (nq, 5))
        sd = torch.from_numpy(seeds).to(g.device)
        run = lambda: g.personalized_pagerank(sd, max_iterations=a.iterations, top_k=a.top_k, as_device=True)      # noqa: E731
        entry = {"call": step(f"{name}-call-{nq}", 300, lambda: windows(torch, run))}
        # the iteration alone: the state of the last call is still in the workspace; 20 steps between two events
        ws, gb = g._ws, g._graph
        st = torch.cuda.current_stream(g.device).cuda_stream

        def steps():
            cur = 0
            for _ in range(a.iterations):
                B.check(lib.rarc_ppr_step(gb.data_ptr(), gb.numel(), n, m, nq, 55706, 0, cur, ws.data_ptr(), ws.numel(), None, st), "rarc_ppr_step")
                cur ^= 1
        wd = torch.ones((nq, 5), dtype=torch.int32, device=g.device)

        def seeded_steps():
            B.check(lib.rarc_ppr_seed(gb.data_ptr(), gb.numel(), n, m, sd.data_ptr(), wd.data_ptr(), nq, 5, ws.data_ptr(), ws.numel(), st),
                    "rarc_ppr_seed")
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            steps()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)
        ms = step(f"{name}-steps-{nq}", 300, lambda: [seeded_steps() for _ in range(5)][2:])
        per_it = statistics.median(ms) / a.iterations
        moved = (2 * m + 4 * n) * nq * 8 + 2 * m * 8 + n * 12      # state rows read and written, adjacency, row pointers, degrees
        entry["iteration_ms"] = round(per_it, 4)
        entry["iteration_bytes"] = moved
        entry["iteration_GBps"] = round(moved / (per_it * 1e-3) / 1e9, 1)
        entry["frac_of_peak_measured"] = round(moved / (per_it * 1e-3) / 1e9 / peak, 4)
        if edges_host is not None:
            secs, how, _ = step(f"{name}-host-{nq}", 900, lambda: host_power_iteration(n, edges_host, seeds, 0.85, a.iterations))
            entry["host"] = {"seconds": round(secs, 4), "how": how}
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
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    peak = step("peak", 120, lambda: stream_read_peak(torch, lib, B, dev))
    res = {"device": torch.cuda.get_device_name(0), "peak_measured_GBps": peak, "limits": PG.limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s"}

    edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
    res["planted_partition"] = bench_graph(torch, lib, B, PG, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges, peak, a)
    del edges
    torch.cuda.empty_cache()

    x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
    pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
    pairs = pairs[:found].contiguous()
    del x
    res["duplicate_groups"] = bench_graph(torch, lib, B, PG, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy(), peak, a)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
