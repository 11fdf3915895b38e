"""k-hop neighbourhoods of the entity graph, on the MI355X (csrc/khop.hip): which entities lie within h hops of a query's
entities, and how far away each is.

What it replaces: the reference keeps entities, events, mentions and relations in Neo4j and leaves every traversal to the
server; a GraphRAG local search over that store gathers an entity's neighbourhood with

    MATCH (s)-[*..h]-(v)

before it collects relations and chunks.  Personalized PageRank does not answer that question — mass is not distance, and PPR
has no notion of "not reachable within h hops", which is what bounds a prompt's context.  Here a batch of up to 256 queries is
one bit-parallel multi-source breadth-first search next to the CSR `rarc_graph_csr` built: one bit per (vertex, query, level).

`EntityGraph.neighbourhood(seeds)` traverses from given seeds, `.expand(index, queries)` takes the seeds from a `FlatIndexF16`
search without leaving HBM, and `.neighbourhood_chunks` / `.expand_chunks` push the neighbourhood through a `MentionMap` onto
the chunks a retriever returns, a mention one hop nearer counting four times as much by default.

The rule is defined in integers (restated by tests/khop_ref.py): the answer is the same bits for any order of the
edges and any batch, and row q of a batch equals the one-query call.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import ctypes

import numpy as np

from ....hip import binding as B

MAX_HOPS = 8                   # levels 0 .. 8 are kept
MAX_SEEDS = 64                 # seed slots per query
MAX_BATCH = 256                # queries per launch; larger batches are cut here
MAX_LIST_VERTICES = 65536      # the longest list per query; the dense levels have no such limit
MAX_DECAY = 1 << 16            # a decay entry
NOT_WITHIN = 255               # the dense level of a vertex that is not within `hops`


def limits() -> dict:
    """The limits of the kernels (csrc/khop.hip): the arguments', and the largest degree walked without splitting the vertex
    across a workgroup."""
    out = (ctypes.c_int * 5)()
    B.check(B.load_library().rarc_khop_limits(out), "rarc_khop_limits")
    return {"max_hops": out[0], "max_batch": out[1], "max_seeds": out[2], "max_vertices": out[3], "split_degree": out[4]}


def default_decay(hops: int) -> np.ndarray:
    """4096 >> (2 h) for h = 0 .. hops: a mention one hop nearer counts four times as much (0 from hop 7 on)"""
    return np.array([4096 >> (2 * h) for h in range(int(hops) + 1)], dtype=np.uint32)


def check_hops(hops, max_vertices=None) -> int:
    """ValueError for negative hops or max_vertices < 1, RarcUnsupported, naming the limit, for what lies above one"""
    if int(hops) != hops or int(hops) < 0:
        raise ValueError(f"hops must be an integer >= 0, got {hops!r}")
    if int(hops) > MAX_HOPS:
        raise B.RarcUnsupported(f"hops={int(hops)}: at most {MAX_HOPS} levels are kept (0 <= hops <= {MAX_HOPS})")
    if max_vertices is not None:
        if int(max_vertices) != max_vertices or int(max_vertices) < 1:
            raise ValueError(f"max_vertices must be an integer >= 1, got {max_vertices!r}")
        if int(max_vertices) > MAX_LIST_VERTICES:
            raise B.RarcUnsupported(f"max_vertices={int(max_vertices)}: a list holds at most 2^16 = {MAX_LIST_VERTICES} vertices; ask for the "
                                    f"dense levels (max_vertices=None) instead")
    return int(hops)


def check_decay(decay, hops: int) -> np.ndarray:
    """-> uint32 [hops + 1]; ValueError for a table of another length or an entry that is no integer in [0, 2^16]"""
    if decay is None:
        return default_decay(hops)
    d = np.asarray(decay)
    if d.shape != (hops + 1,):
        raise ValueError(f"decay must hold hops + 1 = {hops + 1} entries, got an array of shape {d.shape}")
    if not np.all(d == np.floor(d)) or d.min() < 0 or d.max() > MAX_DECAY:
        raise ValueError(f"decay entries must be integers in [0, 2^16 = {MAX_DECAY}]")
    return np.ascontiguousarray(d.astype(np.uint32))


def host_seeds(n: int, seeds) -> np.ndarray:
    """a list of lists of vertices -> int64 [B][s] padded with -1 (s >= 1; an empty list is a query without seeds).  ValueError
    for no queries, more than 64 seeds in a query, or a seed outside [0, n)"""
    rows = [list(r) for r in seeds]
    if not rows:
        raise ValueError("no queries")
    s = max(1, max(len(r) for r in rows))
    if s > MAX_SEEDS:
        raise ValueError(f"{s} seeds in a query: at most {MAX_SEEDS} are taken")
    sd = np.full((len(rows), s), -1, np.int64)
    for i, r in enumerate(rows):
        v = np.asarray(r)
        if v.size and (not np.all(v == np.floor(v)) or v.min() < 0 or v.max() >= n):
            raise ValueError(f"a seed names a vertex outside [0, {n})")
        sd[i, :len(r)] = v
    return sd


def _device_seeds(graph, seeds):
    """seeds as personalized_pagerank takes them -> device int64 [B][s]"""
    t = graph.torch
    if isinstance(seeds, t.Tensor):
        return graph._seed_tensors(seeds, None)[0]
    return t.from_numpy(host_seeds(graph.n, seeds)).to(graph.device)


def _check_mentions(graph, mentions, top_k):
    from .passages import MentionMap

    if not isinstance(mentions, MentionMap):
        raise ValueError("mentions must be a MentionMap")
    if mentions.n_entities != graph.n:
        raise ValueError(f"the mention map is over {mentions.n_entities} entities and the graph has {graph.n} vertices: entity i must be "
                         f"vertex i")
    if mentions.device != graph.device:
        raise ValueError(f"the mention map lives on {mentions.device} and the graph on {graph.device}")
    mentions.check_top_k(top_k)


def traverse(graph, sd, hops: int, early_stop: bool = False):
    """Seeds one launch batch (<= 256 queries) and steps it `hops` times in the graph's k-hop workspace -> (workspace pointer,
    bytes).  early_stop reads the `grew` word after every step and leaves the remaining steps out once it is 0: the levels they
    would write are empty either way."""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq, s = int(sd.shape[0]), int(sd.shape[1])
    need = int(lib.rarc_khop_workspace_bytes(n, m, nq, hops))
    if need == 0:
        raise B.RarcError(f"neighbourhood: n={n}, m={m}, {nq} queries, hops={hops} refused by rarc_khop_workspace_bytes")
    kws = getattr(graph, "_khop_ws", None)
    if kws is None or kws.numel() < need:
        graph._khop_ws = None
        graph._khop_ws = kws = t.empty(need, dtype=t.uint8, device=graph.device)
    ws, wb = kws.data_ptr(), kws.numel()
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_seed(n, m, sd.data_ptr(), nq, s, hops, ws, wb, stream), "rarc_khop_seed")
    grew = t.zeros(1, dtype=t.int32, device=graph.device) if early_stop else None
    for hop in range(1, hops + 1):
        B.check(lib.rarc_khop_step(graph._graph.data_ptr(), graph._graph.numel(), n, m, nq, hops, hop, ws, wb,
                                   grew.data_ptr() if grew is not None else None, stream), "rarc_khop_step")
        if grew is not None and not bool(grew.item()):
            break
    return ws, wb


def _vertices(graph, sd, hops, max_vertices, early_stop):
    """one launch batch -> device tensors: levels uint8 [B][n], or (ids, hops, counts, hop_counts)"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq = int(sd.shape[0])
    ws, wb = traverse(graph, sd, hops, early_stop)
    stream = t.cuda.current_stream(graph.device).cuda_stream
    if max_vertices is None:
        out = t.empty((nq, n), dtype=t.uint8, device=graph.device)
        B.check(lib.rarc_khop_levels(n, m, nq, hops, ws, wb, out.data_ptr(), stream), "rarc_khop_levels")
        return (out,)
    ids = t.empty((nq, max_vertices), dtype=t.int64, device=graph.device)
    hp = t.empty((nq, max_vertices), dtype=t.int32, device=graph.device)
    cnt = t.empty(nq, dtype=t.int32, device=graph.device)
    hc = t.empty((nq, hops + 1), dtype=t.int32, device=graph.device)
    B.check(lib.rarc_khop_list(n, m, nq, hops, max_vertices, ws, wb, ids.data_ptr(), hp.data_ptr(), cnt.data_ptr(), stream), "rarc_khop_list")
    B.check(lib.rarc_khop_counts(n, m, nq, hops, ws, wb, hc.data_ptr(), stream), "rarc_khop_counts")
    return ids, hp, cnt, hc


def _chunks(graph, mentions, sd, hops, decay, top_k, early_stop):
    """one launch batch -> device tensors: scores float64 [B][n_chunks], or (ids, scores, counts)"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq = int(sd.shape[0])
    ws, wb = traverse(graph, sd, hops, early_stop)
    cws, cb = mentions.workspace(nq)
    split, n_split = mentions.split_list()
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_chunks(n, m, nq, hops, decay.ctypes.data, ws, wb, mentions._row_ptr.data_ptr(), mentions._ent.data_ptr(),
                                 mentions._w.data_ptr(), mentions.n_chunks, mentions.nnz, split, n_split, cws, cb, stream), "rarc_khop_chunks")
    out = mentions.ranked(nq, top_k)
    return (out,) if top_k is None else out


def _batched(graph, sd, as_device, one):
    """cuts the queries at 256 per launch batch, runs `one` on each and joins the parts"""
    t = graph.torch
    parts = [one(sd[s0:s0 + MAX_BATCH]) for s0 in range(0, int(sd.shape[0]), MAX_BATCH)]
    out = parts[0] if len(parts) == 1 else tuple(t.cat([p[i] for p in parts]) for i in range(len(parts[0])))
    out = out if as_device else tuple(x.cpu().numpy() for x in out)
    return out[0] if len(out) == 1 else tuple(out)


def neighbourhood(graph, seeds, hops: int = 2, max_vertices=None, as_device: bool = False, early_stop: bool = False):
    hops = check_hops(hops, max_vertices)
    with graph.torch.cuda.device(graph.device):
        sd = _device_seeds(graph, seeds)
        return _batched(graph, sd, as_device, lambda part: _vertices(graph, part, hops, None if max_vertices is None else int(max_vertices),
                                                                      early_stop))


def expand(graph, index, queries, seeds_per_query: int = 5, hops: int = 2, max_vertices=None, as_device: bool = False,
           early_stop: bool = False):
    hops = check_hops(hops, max_vertices)
    graph._check_index(index, seeds_per_query)
    sd, _ = graph._index_seeds(index, queries, seeds_per_query)
    with graph.torch.cuda.device(graph.device):
        return _batched(graph, sd, as_device, lambda part: _vertices(graph, part, hops, None if max_vertices is None else int(max_vertices),
                                                                      early_stop))


def neighbourhood_chunks(graph, mentions, seeds, hops: int = 2, decay=None, top_k=None, as_device: bool = False, early_stop: bool = False):
    hops = check_hops(hops)
    decay = check_decay(decay, hops)
    _check_mentions(graph, mentions, top_k)
    with graph.torch.cuda.device(graph.device):
        sd = _device_seeds(graph, seeds)
        return _batched(graph, sd, as_device, lambda part: _chunks(graph, mentions, part, hops, decay, None if top_k is None else int(top_k),
                                                                    early_stop))


def expand_chunks(graph, index, queries, mentions, seeds_per_query: int = 5, hops: int = 2, decay=None, top_k: int = 10,
                  as_device: bool = False, early_stop: bool = False):
    hops = check_hops(hops)
    decay = check_decay(decay, hops)
    graph._check_index(index, seeds_per_query)
    _check_mentions(graph, mentions, top_k)
    sd, _ = graph._index_seeds(index, queries, seeds_per_query)
    with graph.torch.cuda.device(graph.device):
        return _batched(graph, sd, as_device, lambda part: _chunks(graph, mentions, part, hops, decay, int(top_k), early_stop))


def k_hop(n: int, pairs, seeds, hops: int = 2, device: int = 0, **kw):
    """The one-shot form: EntityGraph(n, pairs, device=device).neighbourhood(seeds, hops, **kw).  The arguments are checked
    before the graph is built: a bad seed, hops or max_vertices raises with no device visible."""
    from .pagerank import EntityGraph

    check_hops(hops, kw.get("max_vertices"))
    if not hasattr(seeds, "is_cuda"):
        host_seeds(int(n), seeds)
    return EntityGraph(n, pairs, device=device).neighbourhood(seeds, hops=hops, **kw)
