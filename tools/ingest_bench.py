#!/usr/bin/env python3
"""Graph ingest on the GPU, timed next to the host route it replaces.  GPU only, one process; every step runs under
its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

The planted-partition graph of tools/merge_bench.py (--vertices vertices, about 4.8 edges per vertex) with the mention map of
tools/passage_bench.py, and the same at --small vertices.  The raw rows are the edges in a random orientation, one in ten repeated,
typed and weighted, shuffled.  Per graph, all in one run:
  * EntityGraph.from_rows and MentionMap.from_rows on device rows;
  * graph.extended and mentions.extended with a batch of 10,000 and of 1,000,000 new rows;
  * rarc_ingest_pairs alone and rarc_merge_pairs alone (an identity map) on the same rows: the same sort over the same keys, so the
    ratio is what the key, mask and writer kernels add;
  * the route replaced: the lists to the host, then the host constructors — one timed run;
  * the lists of both routes are compared before any time is reported.
Device events around the calls, one warm-up, the median and the range of five.

    python3 tools/ingest_bench.py --out profiles/ingest_bench.json
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

from louvain_bench import planted_edges, step  # noqa: E402
from passage_bench import synthetic_mentions  # noqa: E402


def between_events(torch, fn, repeats=5):
    fn()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "calls": repeats}


def raw_rows(edges, seed):
    """the edges as extraction would hand them over: any orientation, one in ten repeated, a type and a weight each, shuffled"""
    rng = np.random.default_rng(seed)
    rows = np.concatenate([edges, edges[rng.integers(0, len(edges), len(edges) // 10)]])
    flip = rng.random(len(rows)) < 0.5
    rows[flip] = rows[flip][:, ::-1]
    rows = rows[rng.permutation(len(rows))]
    return np.ascontiguousarray(rows), rng.integers(1, 10, len(rows)), rng.integers(0, 32, len(rows))


def bench_graph(torch, lib, B, DB, name, n, edges):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    rows, w, t = raw_rows(edges, 5)
    mentions, mw = step(f"{name}-mentions", 300, lambda: synthetic_mentions(n, edges))
    mentions, mw = np.asarray(mentions, np.int64).reshape(-1, 2), np.asarray(mw, np.int64)
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x).astype(dt))).to(dev)         # noqa: E731
    d_rows, d_w, d_t, d_m, d_mw = d(rows, np.int64), d(w, np.int32), d(t, np.int32), d(mentions, np.int64), d(mw, np.int32)
    res = {"vertices": n, "rows": len(rows), "mention_rows": len(mentions)}

    g = DB.EntityGraph.from_rows(n, d_rows, weights=d_w, types=d_t)
    mm = DB.MentionMap.from_rows(n, n, d_m, weights=d_mw)
    res["edges"], res["mentions"] = g.m, mm.nnz
    res["from_rows"] = step(f"{name}-from_rows", 300, lambda: between_events(torch, lambda: DB.EntityGraph.from_rows(n, d_rows, weights=d_w, types=d_t)))
    res["from_rows_untyped_unit"] = step(f"{name}-from_rows-unit", 300, lambda: between_events(torch, lambda: DB.EntityGraph.from_rows(n, d_rows)))
    res["mentions_from_rows"] = step(f"{name}-mentions_from_rows", 300, lambda: between_events(torch, lambda: DB.MentionMap.from_rows(n, n, d_m, weights=d_mw)))
    rng = np.random.default_rng(6)
    for batch in (10_000, 1_000_000):
        br = np.stack([rng.integers(0, n, batch), rng.integers(0, n, batch)], axis=1)
        br = d(br[br[:, 0] != br[:, 1]], np.int64)
        k = int(br.shape[0])
        bw, bt = d(rng.integers(1, 10, k), np.int32), d(rng.integers(0, 32, k), np.int32)
        res[f"extended_{batch}"] = step(f"{name}-extended-{batch}", 300, lambda: between_events(torch, lambda: g.extended(br, weights=bw, types=bt)))
        bm = d(np.stack([rng.integers(0, n, batch), rng.integers(0, n, batch)], axis=1), np.int64)
        res[f"mentions_extended_{batch}"] = step(f"{name}-mentions-extended-{batch}", 300, lambda: between_events(torch, lambda: mm.extended(bm)))

    # ---- the entries alone: rarc_ingest_pairs against rarc_merge_pairs with an identity map, on the same rows
    r = len(rows)
    ws = torch.empty(int(lib.rarc_ingest_pairs_workspace_bytes(0, r)), dtype=torch.uint8, device=dev)
    op, ow, om = torch.empty((r, 2), dtype=torch.int64, device=dev), torch.empty(r, dtype=torch.int32, device=dev), torch.empty(r, dtype=torch.int32, device=dev)
    cnt = torch.empty(8, dtype=torch.int64, device=dev)
    entries = {"ingest_pairs_typed": step(f"{name}-entry", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_ingest_pairs(
        d_rows.data_ptr(), d_w.data_ptr(), d_t.data_ptr(), r, None, None, None, 0, n, ws.data_ptr(), ws.numel(), op.data_ptr(), ow.data_ptr(),
        om.data_ptr(), cnt.data_ptr(), st), "rarc_ingest_pairs")))}
    entries["ingest_pairs_untyped"] = step(f"{name}-entry-untyped", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_ingest_pairs(
        d_rows.data_ptr(), d_w.data_ptr(), None, r, None, None, None, 0, n, ws.data_ptr(), ws.numel(), op.data_ptr(), ow.data_ptr(), None,
        cnt.data_ptr(), st), "rarc_ingest_pairs")))
    del ws
    ws = torch.empty(int(lib.rarc_merge_pairs_workspace_bytes(r)), dtype=torch.uint8, device=dev)
    ident = torch.arange(n, dtype=torch.int64, device=dev)
    entries["merge_pairs"] = step(f"{name}-merge-pairs", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_merge_pairs(
        d_rows.data_ptr(), d_w.data_ptr(), r, ident.data_ptr(), n, ws.data_ptr(), ws.numel(), op.data_ptr(), ow.data_ptr(), cnt.data_ptr(), st),
        "rarc_merge_pairs")))
    del ws, op, ow, om
    entries["typed_over_merge_pairs"] = round(entries["ingest_pairs_typed"]["ms"] / entries["merge_pairs"]["ms"], 3)
    entries["untyped_over_merge_pairs"] = round(entries["ingest_pairs_untyped"]["ms"] / entries["merge_pairs"]["ms"], 3)
    res["entries"] = entries

    # ---- the route replaced: the lists to the host, then the host constructors
    def host_route():
        t0 = time.perf_counter()
        hr, hw, ht = d_rows.cpu().numpy(), d_w.cpu().numpy(), d_t.cpu().numpy()
        hm, hmw = d_m.cpu().numpy(), d_mw.cpu().numpy()
        t1 = time.perf_counter()
        hg = DB.EntityGraph(n, hr, weights=hw, types=ht)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        hmap = DB.MentionMap(n, n, hm, weights=hmw)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return {"to_host_seconds": round(t1 - t0, 4), "entity_graph_seconds": round(t2 - t1, 4), "mention_map_seconds": round(t3 - t2, 4)}, hg, hmap

    host, hg, hmap = step(f"{name}-host", 900, host_route)
    for a, b in ((g._pairs, hg._pairs), (g._pair_weights, hg._pair_weights), (g._type_masks, hg._type_masks), (mm._row_ptr, hmap._row_ptr),
                 (mm._ent, hmap._ent), (mm._w, hmap._w)):
        assert a.shape == b.shape and bool((a == b).all()), "the two routes disagree"
    res["host"] = host
    res["host_graph_over_from_rows"] = round(host["entity_graph_seconds"] * 1e3 / res["from_rows"]["ms"], 1)
    res["host_map_over_from_rows"] = round(host["mention_map_seconds"] * 1e3 / res["mentions_from_rows"]["ms"], 1)
    res["extended_10000_over_from_rows"] = round(res["extended_10000"]["ms"] / res["from_rows"]["ms"], 3)
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--small", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database import graph_db as DB
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    res = {"device": torch.cuda.get_device_name(0), "limits": DB.ingest.limits(),
           "method": "device events around each call (a call ends in the synchronise of its own count read-back), one warm-up, the median, "
                     "minimum and maximum of 5; the host route: one timed run on the host clock"}
    for name, n in (("small", a.small), ("planted_partition", a.vertices)):
        edges = step(f"{name}-edges", 300, lambda: planted_edges(n, 20, 0.5, 0.1, 2))
        res[name] = bench_graph(torch, lib, B, DB, name, n, edges)
        torch.cuda.empty_cache()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
