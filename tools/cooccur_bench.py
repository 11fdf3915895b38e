#!/usr/bin/env python3
"""The co-occurrence projection on the GPU, timed next to the host route it replaces.  GPU only, one process; every
step runs under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

The two mention maps of tools/passage_bench.py: n chunks over the n entities of the duplicate-group graph of --rows x 768 Gaussian
rows, and of the planted-partition edge list of --vertices vertices (1,000,000 chunks, about 4.5 M mentions).  Per map:
  * each of rarc_cooccur_count, rarc_cooccur_emit, rarc_sort_reduce and rarc_cooccur_edges alone, between two device events: one
    warm-up, then the median of --repeats with the range; EntityGraph.from_device (the CSR build) by the host clock around a call
    that ends in a synchronise, the same way;
  * MentionMap.cooccurrence() end to end, the resident EntityGraph included: ms per call by the method of tools/ppr_bench.py;
  * the host route it replaces, in the same run: the mention CSR to the host, the upper triangle of AᵀA in scipy.sparse (np.unique
    over the expanded pairs where scipy is absent), EntityGraph(n, pairs, weights) from host arrays; one timed run;
  * the pair lists and weights of both routes are compared before any time is reported.

    python3 tools/cooccur_bench.py --out profiles/cooccur_bench.json
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
from ppr_bench import windows  # noqa: E402


def spread(ms):
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "repeats": len(ms)}


def between_events(torch, fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return spread(out)


def host_clock(torch, fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def host_route(DB, mm, weight):
    """-> (seconds by part, the EntityGraph) — what a caller did before MentionMap.cooccurrence"""
    n = mm.n_entities
    t0 = time.perf_counter()
    row_ptr, ent, w = mm._row_ptr.cpu().numpy(), mm._ent.cpu().numpy().astype(np.int64), mm._w.cpu().numpy().view(np.uint32).astype(np.int64)
    t1 = time.perf_counter()
    deg = np.diff(row_ptr)
    chunk = np.repeat(np.arange(mm.n_chunks), deg)
    data = np.ones(len(ent), np.int64) if weight == "count" else w
    try:
        import scipy.sparse as sp

        a = sp.csr_matrix((data, (chunk, ent)), shape=(mm.n_chunks, n))
        gram = sp.triu(a.T @ a, k=1).tocoo()
        pairs, weights = np.stack([gram.row, gram.col], axis=1).astype(np.int64), gram.data.astype(np.int64)
        how = "scipy.sparse: triu(A.T @ A, 1)"
    except ImportError:
        rows = [(ent[r0:r1], data[r0:r1]) for r0, r1 in zip(row_ptr[:-1], row_ptr[1:]) if r1 - r0 >= 2]
        ij = [np.triu_indices(len(e), k=1) for e, _ in rows]
        a = np.concatenate([e[i] for (e, _), (i, _) in zip(rows, ij)])
        b = np.concatenate([e[j] for (e, _), (_, j) in zip(rows, ij)])
        v = np.concatenate([x[i] * x[j] for (_, x), (i, j) in zip(rows, ij)])
        pairs, inv = np.unique(np.stack([a, b], axis=1), axis=0, return_inverse=True)
        weights = np.bincount(inv.ravel(), weights=v.astype(np.float64), minlength=len(pairs)).astype(np.int64)
        how = "numpy: np.triu_indices per chunk, np.unique(axis=0) + bincount"
    t2 = time.perf_counter()
    g = DB.EntityGraph(n, pairs, weights=weights)
    import torch

    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"seconds": round(t3 - t0, 4), "to_host_seconds": round(t1 - t0, 4), "project_seconds": round(t2 - t1, 4),
            "host_constructor_seconds": round(t3 - t2, 4), "how": f"device -> host, {how}, EntityGraph host constructor"}, g


def bench_map(torch, lib, B, DB, name, n, edges_host, a):
    mentions, weights = step(f"{name}-mentions", 300, lambda: synthetic_mentions(n, edges_host))
    mm = step(f"{name}-map", 300, lambda: DB.MentionMap(n, n, mentions, weights))
    dev = mm.device
    st = torch.cuda.current_stream(dev).cuda_stream
    nc, nnz = mm.n_chunks, mm.nnz
    res = {"chunks": nc, "entities": n, "mentions": nnz, "weight": a.weight, "max_mentions": a.max_mentions}
    mode = {"count": 0, "product": 1}[a.weight]
    csr = (mm._row_ptr.data_ptr(), mm._ent.data_ptr(), mm._w.data_ptr(), nc, nnz, n)

    # ---- the entries alone
    def alone(what, call):
        return step(f"{name}-{what}", 120, lambda: between_events(torch, call, a.repeats))

    ws = torch.empty(int(lib.rarc_cooccur_workspace_bytes(nc, nnz)), dtype=torch.uint8, device=dev)
    out4 = torch.empty(4, dtype=torch.int64, device=dev)
    steps = {"count": alone("count", lambda: B.check(lib.rarc_cooccur_count(*csr, a.max_mentions, ws.data_ptr(), ws.numel(), out4.data_ptr(), st),
                                                     "rarc_cooccur_count"))}
    total, contributing, over, skipped = out4.tolist()
    res.update({"total_pairs": total, "contributing_chunks": contributing, "chunks_skipped": over, "entries_skipped": skipped})
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    values = torch.empty(total, dtype=torch.int32, device=dev) if mode else None
    vp = values.data_ptr() if mode else None
    steps["emit"] = alone("emit", lambda: B.check(lib.rarc_cooccur_emit(*csr, mode, ws.data_ptr(), ws.numel(), keys.data_ptr(), vp, total, st),
                                                  "rarc_cooccur_emit"))
    steps["emit"]["written_gb_per_s"] = round(total * (12 if mode else 8) / steps["emit"]["ms"] / 1e6, 1)
    sws = torch.empty(int(lib.rarc_sort_reduce_workspace_bytes(total)), dtype=torch.uint8, device=dev)
    uk, us, out2 = (torch.empty(k, dtype=torch.int64, device=dev) for k in (total, total, 2))
    key_bits = 2 * max(1, (n - 1).bit_length())
    steps["sort_reduce"] = alone("sort", lambda: B.check(lib.rarc_sort_reduce(keys.data_ptr(), vp, total, key_bits, sws.data_ptr(), sws.numel(),
                                                                              uk.data_ptr(), us.data_ptr(), out2.data_ptr(), st), "rarc_sort_reduce"))
    steps["sort_reduce"].update({"key_bits": key_bits, "passes": (key_bits + 7) // 8})
    distinct = int(out2[0].item())
    ews = torch.empty(int(lib.rarc_cooccur_edges_workspace_bytes(distinct)), dtype=torch.uint8, device=dev)
    pairs, w = torch.empty((distinct, 2), dtype=torch.int64, device=dev), torch.empty(distinct, dtype=torch.int32, device=dev)
    out3 = torch.empty(3, dtype=torch.int64, device=dev)
    steps["edges"] = alone("edges", lambda: B.check(lib.rarc_cooccur_edges(uk.data_ptr(), us.data_ptr(), distinct, n, a.min_weight, ews.data_ptr(),
                                                                           ews.numel(), pairs.data_ptr(), w.data_ptr(), out3.data_ptr(), st),
                                                    "rarc_cooccur_edges"))
    m, largest, below = out3.tolist()
    res.update({"distinct_edges": m, "largest_weight": largest, "below_min_weight": below})
    del ws, keys, values, sws, uk, us, ews
    steps["from_device"] = step(f"{name}-csr", 120, lambda: host_clock(torch, lambda: DB.EntityGraph.from_device(n, pairs[:m], w[:m]), a.repeats))
    res["steps"] = steps
    res["steps_sum_ms"] = round(sum(s["ms"] for s in steps.values()), 4)

    # ---- end to end, and the host route
    run = lambda: mm.cooccurrence(weight=a.weight, min_weight=a.min_weight, max_mentions=a.max_mentions)      # noqa: E731
    res["cooccurrence"] = step(f"{name}-call", 300, lambda: windows(torch, run))
    got = run()
    host, hg = step(f"{name}-host", 900, lambda: host_route(DB, mm, a.weight))
    for x, y in ((got._pairs, hg._pairs), (got._pair_weights, hg._pair_weights)):
        assert x.shape == y.shape and bool((x == y).all()), "the two routes disagree"
    res["host"] = host
    res["call_faster_than_host_route"] = bool(res["cooccurrence"]["ms"] * 1e-3 < host["seconds"])
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--maps", default="duplicate_groups,planted_partition")
    ap.add_argument("--weight", default="count", choices=("count", "product"))
    ap.add_argument("--min-weight", type=int, default=1)
    ap.add_argument("--max-mentions", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database import graph_db as DB
    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence as CO
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "limits": CO.limits(),
           "method": "an entry alone: device events around one launch group, one warm-up, the median of `repeats` with the range; from_device: "
                     "host clock around a call ending in a synchronise, the same way; cooccurrence: ms per call, host clock around calls ending "
                     "in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; the host route: one timed run"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "duplicate_groups" in a.maps:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        edges = pairs[:found].cpu().numpy()
        del x, pairs
        torch.cuda.empty_cache()
        res["duplicate_groups"] = bench_map(torch, lib, B, DB, "duplicate_groups", a.rows, edges, a)
        torch.cuda.empty_cache()
        save()
    if "planted_partition" in a.maps:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_map(torch, lib, B, DB, "planted_partition", a.vertices, edges, a)
        save()


if __name__ == "__main__":
    main()
