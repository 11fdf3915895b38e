#!/usr/bin/env python3
"""Entity merging on the GPU, timed next to the host route it replaces.  GPU only, one process; every step runs
under its own time limit (SIGALRM: a step that overruns ends the process — nothing more is started behind a hang).

The two graphs of tools/khop_edges_bench.py (the planted-partition edge list of --vertices vertices, about 4.8 edges per vertex,
and the duplicate-group graph of --rows x 768 Gaussian rows), each with the mention map of tools/passage_bench.py (n chunks over
the n entities), its own pair list as the relation table, and planted labels that merge about 4 % of the vertices into groups of
2 .. 4.  Per graph:
  * rarc_sort_reduce alone on the pair keys (min << bits(n) | max), between two events, the median of five: at the pair key's
    own width, and at 8, 16, ... bits (keys masked to that width) — the differences are the passes;
  * each of rarc_merge_plan, rarc_merge_pairs, rarc_merge_mentions, rarc_merge_relations alone, the same way;
  * merge_entities(labels, graph, mentions, relations) end to end, new resident objects included: ms per call by the method of
    tools/ppr_bench.py (the `method` string records it);
  * the host route it replaces, in the same run: the pair list, the CSR and the relation table to the host, numpy relabel +
    np.unique / bincount, and the existing host constructors (which upload again); one timed run;
  * the buffers of both routes are compared before any time is reported.

    python3 tools/merge_bench.py --out profiles/merge_bench.json
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


def planted_labels(n, fraction, seed):
    """labels int64 [n]: about `fraction` of the vertices in groups of 2 .. 4, each labelled by a random member"""
    rng = np.random.default_rng(seed)
    labels = np.arange(n, dtype=np.int64)
    perm = rng.permutation(n)[:int(n * fraction)]
    at = 0
    while at + 4 <= len(perm):
        size = int(rng.integers(2, 5))
        labels[perm[at:at + size]] = perm[at + int(rng.integers(size))]
        at += size
    return labels


def between_events(torch, fn):
    fn()
    out = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return round(statistics.median(out), 4)


def host_route(DB, PS, n, labels, rich, g, mm, rl):
    """-> (seconds by part, the three objects) — what a caller did before merge_entities"""
    t0 = time.perf_counter()
    pairs, w = g._pairs.cpu().numpy(), None if g._pair_weights is None else g._pair_weights.cpu().numpy().view(np.uint32).astype(np.int64)
    row_ptr, ent, mw = mm._row_ptr.cpu().numpy(), mm._ent.cpu().numpy(), mm._w.cpu().numpy().view(np.uint32)
    rel = rl._pairs.cpu().numpy()
    t1 = time.perf_counter()
    order = np.lexsort((np.arange(n), -rich, labels))                      # the plan (tests/merge_ref.py)
    lo = labels[order]
    first = np.ones(n, bool)
    first[1:] = lo[1:] != lo[:-1]
    best = np.full(n, -1, np.int64)
    best[lo[first]] = order[first]
    primary = best[labels]
    kept = np.flatnonzero(primary == np.arange(n))
    number = np.full(n, -1, np.int64)
    number[kept] = np.arange(len(kept))
    new_id = number[primary]
    t2 = time.perf_counter()
    a, b = new_id[pairs[:, 0]], new_id[pairs[:, 1]]
    keep = a != b
    up, inv = np.unique(np.stack([np.minimum(a, b)[keep], np.maximum(a, b)[keep]], axis=1), axis=0, return_inverse=True)
    uw = np.bincount(inv.ravel(), weights=(np.ones(len(pairs)) if w is None else w.astype(np.float64))[keep], minlength=len(up)).astype(np.int64)
    chunk = np.repeat(np.arange(mm.n_chunks), np.diff(row_ptr))
    ment = np.stack([chunk, new_id[ent]], axis=1)
    ra, rb = new_id[rel[:, 0]], new_id[rel[:, 1]]
    stay = (rel[:, 0] == rel[:, 1]) | (ra != rb)
    table = np.stack([ra[stay], rb[stay]], axis=1)
    t3 = time.perf_counter()
    objs = (DB.EntityGraph(len(kept), up, weights=uw), DB.MentionMap(mm.n_chunks, len(kept), ment, mw.astype(np.int64)),
            DB.RelationList(len(kept), table))
    import torch

    torch.cuda.synchronize()
    t4 = time.perf_counter()
    return {"seconds": round(t4 - t0, 4), "to_host_seconds": round(t1 - t0, 4), "plan_seconds": round(t2 - t1, 4),
            "relabel_unique_seconds": round(t3 - t2, 4), "host_constructors_seconds": round(t4 - t3, 4),
            "how": "device -> host, numpy plan, relabel + np.unique(axis=0) / bincount, EntityGraph / MentionMap / RelationList host constructors"}, objs


def bench_graph(torch, lib, B, DB, PS, MG, name, n, pairs_dev, edges_host):
    g = DB.EntityGraph(n, pairs_dev)
    m = g.m
    mentions, weights = step(f"{name}-mentions", 300, lambda: synthetic_mentions(n, edges_host))
    mm = step(f"{name}-map", 300, lambda: PS.MentionMap(n, n, mentions, weights))
    rl = DB.RelationList(n, g._pairs)
    labels = planted_labels(n, 0.04, 3)
    rich = np.random.default_rng(4).integers(0, 50, n)
    dev = g.device
    st = torch.cuda.current_stream(dev).cuda_stream
    res = {"vertices": n, "edges": m, "mentions": mm.nnz, "chunks": mm.n_chunks, "relations": rl.r}
    plan = MG.merge_plan(torch.from_numpy(labels).to(dev), torch.from_numpy(rich).to(dev), as_device=True)
    res["merged_vertices"] = n - plan.n_merged

    # ---- rarc_sort_reduce alone, on the pair keys
    bits = max(1, int(n - 1).bit_length())
    keys = (torch.minimum(g._pairs[:, 0], g._pairs[:, 1]) << bits) | torch.maximum(g._pairs[:, 0], g._pairs[:, 1])
    ws = torch.empty(int(lib.rarc_sort_reduce_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    ok, osum, out2 = (torch.empty(k, dtype=torch.int64, device=dev) for k in (m, m, 2))
    sort = {"key_bits": 2 * bits, "passes": (2 * bits + 7) // 8, "workspace_bytes": ws.numel(), "by_key_bits_ms": {}}
    for kb in sorted(set(range(8, 2 * bits, 8)) | {2 * bits}):
        kk = (keys & ((1 << kb) - 1)).contiguous()
        sort["by_key_bits_ms"][str(kb)] = step(f"{name}-sort-{kb}", 120, lambda: between_events(torch, lambda: B.check(lib.rarc_sort_reduce(
            kk.data_ptr(), None, m, kb, ws.data_ptr(), ws.numel(), ok.data_ptr(), osum.data_ptr(), out2.data_ptr(), st), "rarc_sort_reduce")))
    ladder = [sort["by_key_bits_ms"][k] for k in sorted(sort["by_key_bits_ms"], key=int)]
    sort["total_ms"] = ladder[-1]
    sort["ms_per_pass"] = round((ladder[-1] - ladder[0]) / max(1, sort["passes"] - 1), 4) if len(ladder) > 1 else ladder[0]
    sort["reduce_and_first_pass_ms"] = ladder[0]
    res["sort_reduce"] = sort
    del ws, ok, osum, keys

    # ---- the four entries alone
    def alone(what, call):
        return step(f"{name}-{what}", 120, lambda: between_events(torch, call))

    lab_d, rich_d = torch.from_numpy(labels).to(dev), torch.from_numpy(rich.astype(np.uint32).view(np.int32)).to(dev)
    pws = torch.empty(int(lib.rarc_merge_plan_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    o = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    cnt = torch.empty(8, dtype=torch.int64, device=dev)
    entries = {"plan_ms": alone("plan", lambda: B.check(lib.rarc_merge_plan(lab_d.data_ptr(), rich_d.data_ptr(), n, pws.data_ptr(), pws.numel(),
                                                                            o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(),
                                                                            cnt.data_ptr(), st), "rarc_merge_plan"))}
    new_id = plan._new_id
    ws = torch.empty(int(lib.rarc_merge_pairs_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    op, ow = torch.empty((m, 2), dtype=torch.int64, device=dev), torch.empty(m, dtype=torch.int32, device=dev)
    entries["pairs_ms"] = alone("pairs", lambda: B.check(lib.rarc_merge_pairs(g._pairs.data_ptr(), None, m, new_id.data_ptr(), n, ws.data_ptr(),
                                                                              ws.numel(), op.data_ptr(), ow.data_ptr(), cnt.data_ptr(), st),
                                                         "rarc_merge_pairs"))
    del ws, op, ow
    ws = torch.empty(int(lib.rarc_merge_mentions_workspace_bytes(mm.n_chunks, mm.nnz)), dtype=torch.uint8, device=dev)
    orp = torch.empty(mm.n_chunks + 1, dtype=torch.int64, device=dev)
    oe, ow, osp = (torch.empty(k, dtype=torch.int32, device=dev) for k in (mm.nnz, mm.nnz, mm.n_chunks))
    entries["mentions_ms"] = alone("mentions", lambda: B.check(lib.rarc_merge_mentions(
        mm._row_ptr.data_ptr(), mm._ent.data_ptr(), mm._w.data_ptr(), mm.n_chunks, mm.nnz, new_id.data_ptr(), n, ws.data_ptr(), ws.numel(),
        orp.data_ptr(), oe.data_ptr(), ow.data_ptr(), osp.data_ptr(), cnt.data_ptr(), st), "rarc_merge_mentions"))
    del ws, orp, oe, ow, osp
    ws = torch.empty(int(lib.rarc_merge_relations_workspace_bytes(rl.r)), dtype=torch.uint8, device=dev)
    orel, orow = torch.empty((rl.r, 2), dtype=torch.int64, device=dev), torch.empty(rl.r, dtype=torch.int64, device=dev)
    entries["relations_ms"] = alone("relations", lambda: B.check(lib.rarc_merge_relations(
        rl._pairs.data_ptr(), rl.r, new_id.data_ptr(), n, ws.data_ptr(), ws.numel(), orel.data_ptr(), orow.data_ptr(), cnt.data_ptr(), st),
        "rarc_merge_relations"))
    del ws, orel, orow
    res["entries"] = entries

    # ---- end to end, and the host route
    res["merge_entities"] = step(f"{name}-call", 300, lambda: windows(
        torch, lambda: MG.merge_entities(lab_d, graph=g, mentions=mm, relations=rl, richness=torch.from_numpy(rich).to(dev), as_device=True)))
    got = MG.merge_entities(labels, graph=g, mentions=mm, relations=rl, richness=rich)
    host, (hg, hm, hr) = step(f"{name}-host", 900, lambda: host_route(DB, PS, n, labels, rich, g, mm, rl))
    for a, b in ((got.graph._pairs, hg._pairs), (got.graph._pair_weights, hg._pair_weights), (got.mentions._row_ptr, hm._row_ptr),
                 (got.mentions._ent, hm._ent), (got.mentions._w, hm._w), (got.relations._pairs, hr._pairs)):
        assert a.shape == b.shape and bool((a == b).all()), "the two routes disagree"
    res["host"] = host
    res["merged_edges"], res["merged_mentions"], res["merged_relations"], res["dropped"] = got.graph.m, got.mentions.nnz, got.relations.r, got.dropped
    res["call_faster_than_host_route"] = bool(res["merge_entities"]["ms"] * 1e-3 < host["seconds"])
    print(json.dumps({name: res}), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--vertices", type=int, default=1000000)
    ap.add_argument("--graphs", default="duplicate_groups,planted_partition")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from rag_arc_amd.encapsulation.database import graph_db as DB
    from rag_arc_amd.encapsulation.database.graph_db import merge as MG
    from rag_arc_amd.encapsulation.database.graph_db import passages as PS
    from rag_arc_amd.encapsulation.database.graph_db import similarity as S
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "limits": MG.limits(),
           "method": "ms per call: host clock around calls ending in a synchronise, 2 warm-up calls, median of 3 windows of >= 0.25 s; "
                     "an entry alone: device events around one launch group, one warm-up, the median of 5; the host route: one timed run"}

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    if "duplicate_groups" in a.graphs:
        x, _ = step("rows", 120, lambda: make_rows(torch, a.rows, a.dim, 1))
        pairs, _, found = step("pairs", 300, lambda: S._pairs_on_device(lib, x, 0.95, dev))
        pairs = pairs[:found].contiguous()
        del x
        res["duplicate_groups"] = bench_graph(torch, lib, B, DB, PS, MG, "duplicate_groups", a.rows, pairs, pairs.cpu().numpy())
        del pairs
        torch.cuda.empty_cache()
        save()
    if "planted_partition" in a.graphs:
        edges = step("edges", 300, lambda: planted_edges(a.vertices, 20, 0.5, 0.1, 2))
        res["planted_partition"] = bench_graph(torch, lib, B, DB, PS, MG, "planted_partition", a.vertices, torch.from_numpy(edges).to(dev), edges)
        save()


if __name__ == "__main__":
    main()
