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
the chunks a retriever returns, a mention one hop nearer counting four times as much by default.  `.subgraph` /
`.neighbourhood_edges` / `.expand_subgraph` add the third thing a local search collects, MATCH (a)-[r]-(b) WHERE a, b IN nodes:
the rows of a `RelationList` (the caller's typed relations, or the graph's own pairs) whose two ends both lie in the
neighbourhood, from the same traversal.  `.shortest_paths` / `.path_chunks` / `.connect` answer the other
question a multi-hop query asks, MATCH p = allShortestPaths((a)-[*..L]-(b)): the vertices and relations on every shortest path
between two sources of one traversal, written as a k-hop state of their own so that the lists, the relation rows and the chunk
projection read it unchanged.

The rule is defined in integers (restated by tests/khop_ref.py): the answer is the same bits for any order of the
edges and any batch, and row q of a batch equals the one-query call.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from ....hip import binding as B

MAX_LIST_EDGES = 65536         # the longest relation list per query; edge_level_counts is never cut
MAX_RELATIONS = (1 << 31) - 1  # rows of a relation table: r < 2^31 - 1
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


# ---- typed traversal: the relation types a query may cross (restated by tests/typed_ref.py) ------------------------------
MAX_TYPES = 32                 # a type is an integer in [0, 32): a bit of an edge's mask and of a query's filter


def type_mask(types) -> int:
    """an iterable of type ids -> the uint32 with their bits; ValueError for an id that is no integer in [0, 32)"""
    mask = 0
    for x in types:
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or not 0 <= int(x) < MAX_TYPES:
            raise ValueError(f"a relation type must be an integer in [0, {MAX_TYPES}), got {x!r}")
        mask |= 1 << int(x)
    return mask


def check_type_ids(types, count: int, what: str) -> np.ndarray:
    """one type id per row -> int32 [count]; ValueError for another length or an id outside [0, 32)"""
    a = np.asarray(types)
    if a.shape != (count,):
        raise ValueError(f"expected {count} types, one per {what}, got an array of shape {a.shape}")
    if a.dtype == np.bool_ or (count and not np.all(a == np.floor(a))) or (count and (a.min() < 0 or a.max() >= MAX_TYPES)):
        raise ValueError(f"a relation type must be an integer in [0, {MAX_TYPES})")
    return np.ascontiguousarray(a.astype(np.int32))


def host_filters(relation_types) -> np.ndarray:
    """relation_types as the query calls take it -> uint32 [k] of filters, k >= 1: a uint32 array [k] of masks as it is, one
    iterable of type ids as one filter, a sequence of k iterables as k filters.  ValueError for an id outside [0, 32) or no
    filter at all"""
    if isinstance(relation_types, np.ndarray) and relation_types.dtype == np.uint32:
        if relation_types.ndim != 1 or relation_types.shape[0] < 1:
            raise ValueError(f"filter masks must be a uint32 array [B], got an array of shape {relation_types.shape}")
        return np.ascontiguousarray(relation_types)
    if isinstance(relation_types, (str, bytes)) or not hasattr(relation_types, "__iter__"):
        raise ValueError(f"relation_types must be None, an iterable of type ids, a sequence of them or a uint32 array of masks, got "
                         f"{relation_types!r}")
    rows = list(relation_types)
    if all(not hasattr(x, "__iter__") for x in rows):                                        # one filter for every query (an empty one: F = 0)
        return np.array([type_mask(rows)], np.uint32)
    if any(not hasattr(x, "__iter__") or isinstance(x, (str, bytes)) for x in rows):
        raise ValueError("relation_types mixes type ids and filters: give one iterable of ids, or one iterable per query")
    return np.array([type_mask(x) for x in rows], np.uint32)


def spread_filters(filters: np.ndarray, nq: int) -> np.ndarray:
    """uint32 [1] or [nq] -> uint32 [nq]; ValueError for another count"""
    if filters.shape[0] == nq:
        return filters
    if filters.shape[0] != 1:
        raise ValueError(f"{filters.shape[0]} filters for {nq} queries: relation_types holds one filter for all of them or one per query")
    return np.repeat(filters, nq)


def check_typed(graph, relation_types):
    """-> None for relation_types=None (the untyped traversal), else host_filters(); ValueError on a graph without masks"""
    if relation_types is None:
        return None
    if not graph.typed:
        raise ValueError("relation_types on a graph without type masks: build it with EntityGraph(..., types=), from_relations() or "
                         "from_device(type_masks=)")
    return host_filters(relation_types)


def _device_filters(graph, filters, nq: int):
    """host filters (or None) -> device int32 [nq] holding the uint32 bits (or None)"""
    if filters is None:
        return None
    return graph.torch.from_numpy(spread_filters(filters, nq).view(np.int32)).to(graph.device)


def _single_filter(graph, relation_types):
    """the filter of a paths call: None, or uint32 [1]; ValueError for per-query filters"""
    filters = check_typed(graph, relation_types)
    if filters is not None and filters.shape[0] != 1:
        raise ValueError(f"{filters.shape[0]} filters on a paths call: hop_A(v) + hop_B(v) == d needs every source under one filter, give "
                         f"one iterable of type ids")
    return filters


def typed_adjacency(graph, weighted: bool = False):
    """The graph's typed slot arrays (rarc_graph_types), built on the first typed call and kept -> the device buffer.
    weighted: the same arrays with their weight plane behind them (rarc_graph_types_weighted), built on the first
    typed PPR call and kept; from then on the k-hop entries are handed its prefix, so a graph holds one copy of the planes"""
    tw = getattr(graph, "_typed_adj_weighted", None)
    if weighted and tw is None:
        t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
        need, prefix = int(lib.rarc_graph_types_weighted_workspace_bytes(n, m)), int(lib.rarc_graph_types_workspace_bytes(n, m))
        if need == 0:
            raise B.RarcError(f"typed PageRank: n={n}, m={m} refused by rarc_graph_types_weighted_workspace_bytes")
        tw = t.empty(need, dtype=t.uint8, device=graph.device)
        stream = t.cuda.current_stream(graph.device).cuda_stream
        pw = graph._pair_weights
        B.check(lib.rarc_graph_types_weighted(graph._graph.data_ptr(), graph._graph.numel(), n, m, graph._pairs.data_ptr(),
                                              graph._type_masks.data_ptr(), pw.data_ptr() if pw is not None else None, tw.data_ptr(), tw.numel(),
                                              stream), "rarc_graph_types_weighted")
        graph._typed_adj_weighted = tw
        graph._typed_adj = tw[:prefix]                                  # (an unweighted blob built earlier is let go)
    if weighted:
        return tw
    ta = getattr(graph, "_typed_adj", None)
    if ta is None:
        t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
        need = int(lib.rarc_graph_types_workspace_bytes(n, m))
        if need == 0:
            raise B.RarcError(f"typed traversal: n={n}, m={m} refused by rarc_graph_types_workspace_bytes")
        ta = t.empty(need, dtype=t.uint8, device=graph.device)
        stream = t.cuda.current_stream(graph.device).cuda_stream
        B.check(lib.rarc_graph_types(graph._graph.data_ptr(), graph._graph.numel(), n, m, graph._pairs.data_ptr(), graph._type_masks.data_ptr(),
                                     ta.data_ptr(), ta.numel(), stream), "rarc_graph_types")
        graph._typed_adj = ta
    return ta


def traverse(graph, sd, hops: int, early_stop: bool = False, filters=None):
    """Seeds one launch batch (<= 256 queries) and steps it `hops` times in the graph's k-hop workspace -> (workspace pointer,
    bytes).  early_stop reads the `grew` word after every step and leaves the remaining steps out once it is 0: the levels they
    would write are empty either way.  filters: None, or a device int32 [nq] of uint32 filters — the typed step, same state."""
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
    ta = typed_adjacency(graph) if filters is not None and hops else None
    for hop in range(1, hops + 1):
        if filters is None:
            B.check(lib.rarc_khop_step(graph._graph.data_ptr(), graph._graph.numel(), n, m, nq, hops, hop, ws, wb,
                                       grew.data_ptr() if grew is not None else None, stream), "rarc_khop_step")
        else:
            B.check(lib.rarc_khop_step_typed(graph._graph.data_ptr(), graph._graph.numel(), ta.data_ptr(), ta.numel(), filters.data_ptr(), n, m,
                                             nq, hops, hop, ws, wb, grew.data_ptr() if grew is not None else None, stream),
                    "rarc_khop_step_typed")
        if grew is not None and not bool(grew.item()):
            break
    return ws, wb


def _vertices(graph, sd, hops, max_vertices, early_stop, filters=None):
    """one launch batch -> device tensors: levels uint8 [B][n], or (ids, hops, counts, hop_counts)"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq = int(sd.shape[0])
    ws, wb = traverse(graph, sd, hops, early_stop, filters)
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


def _chunks(graph, mentions, sd, hops, decay, top_k, early_stop, filters=None):
    """one launch batch -> device tensors: scores float64 [B][n_chunks], or (ids, scores, counts)"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq = int(sd.shape[0])
    ws, wb = traverse(graph, sd, hops, early_stop, filters)
    cws, cb = mentions.workspace(nq)
    split, n_split = mentions.split_list()
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_chunks(n, m, nq, hops, decay.ctypes.data, ws, wb, mentions._row_ptr.data_ptr(), mentions._ent.data_ptr(),
                                 mentions._w.data_ptr(), mentions.n_chunks, mentions.nnz, split, n_split, cws, cb, stream), "rarc_khop_chunks")
    out = mentions.ranked(nq, top_k)
    return (out,) if top_k is None else out


def _batched(graph, sd, as_device, one, filters=None):
    """cuts the queries at 256 per launch batch, and the host `filters` (None: untyped) with them, runs `one(seeds, device
    filters)` on each and joins the parts"""
    t = graph.torch
    fd = _device_filters(graph, filters, int(sd.shape[0]))
    parts = [one(sd[s0:s0 + MAX_BATCH], None if fd is None else fd[s0:s0 + MAX_BATCH]) for s0 in range(0, int(sd.shape[0]), MAX_BATCH)]
    out = parts[0] if len(parts) == 1 else tuple(t.cat([p[i] for p in parts]) for i in range(len(parts[0])))
    out = out if as_device else tuple(x.cpu().numpy() for x in out)
    return out[0] if len(out) == 1 else tuple(out)


def neighbourhood(graph, seeds, hops: int = 2, max_vertices=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
    hops = check_hops(hops, max_vertices)
    filters = check_typed(graph, relation_types)
    with graph.torch.cuda.device(graph.device):
        sd = _device_seeds(graph, seeds)
        return _batched(graph, sd, as_device, lambda part, f: _vertices(graph, part, hops, None if max_vertices is None else int(max_vertices),
                                                                         early_stop, f), filters)


def expand(graph, index, queries, seeds_per_query: int = 5, hops: int = 2, max_vertices=None, as_device: bool = False,
           early_stop: bool = False, relation_types=None):
    hops = check_hops(hops, max_vertices)
    filters = check_typed(graph, relation_types)
    graph._check_index(index, seeds_per_query)
    sd, _ = graph._index_seeds(index, queries, seeds_per_query)
    with graph.torch.cuda.device(graph.device):
        return _batched(graph, sd, as_device, lambda part, f: _vertices(graph, part, hops, None if max_vertices is None else int(max_vertices),
                                                                         early_stop, f), filters)


def neighbourhood_chunks(graph, mentions, seeds, hops: int = 2, decay=None, top_k=None, as_device: bool = False, early_stop: bool = False,
                         relation_types=None):
    hops = check_hops(hops)
    decay = check_decay(decay, hops)
    filters = check_typed(graph, relation_types)
    _check_mentions(graph, mentions, top_k)
    with graph.torch.cuda.device(graph.device):
        sd = _device_seeds(graph, seeds)
        return _batched(graph, sd, as_device, lambda part, f: _chunks(graph, mentions, part, hops, decay, None if top_k is None else int(top_k),
                                                                       early_stop, f), filters)


def expand_chunks(graph, index, queries, mentions, seeds_per_query: int = 5, hops: int = 2, decay=None, top_k: int = 10,
                  as_device: bool = False, early_stop: bool = False, relation_types=None):
    hops = check_hops(hops)
    decay = check_decay(decay, hops)
    filters = check_typed(graph, relation_types)
    graph._check_index(index, seeds_per_query)
    _check_mentions(graph, mentions, top_k)
    sd, _ = graph._index_seeds(index, queries, seeds_per_query)
    with graph.torch.cuda.device(graph.device):
        return _batched(graph, sd, as_device, lambda part, f: _chunks(graph, mentions, part, hops, decay, int(top_k), early_stop, f), filters)


# ---- subgraphs: the relations inside the neighbourhood (restated by tests/subgraph_ref.py) --------------------------------
def edges_limits() -> dict:
    """The limits of rarc_khop_edges: the longest list per query, and the rows a tile of its count / scan / write passes holds."""
    out = (ctypes.c_int * 2)()
    B.check(B.load_library().rarc_khop_edges_limits(out), "rarc_khop_edges_limits")
    return {"max_edges": out[0], "tile": out[1]}


def check_max_edges(max_edges) -> int:
    """ValueError for max_edges < 1, RarcUnsupported, naming the limit, above 65536"""
    if int(max_edges) != max_edges or int(max_edges) < 1:
        raise ValueError(f"max_edges must be an integer >= 1, got {max_edges!r}")
    if int(max_edges) > MAX_LIST_EDGES:
        raise B.RarcUnsupported(f"max_edges={int(max_edges)}: a list holds at most 2^16 = {MAX_LIST_EDGES} relations; edge_level_counts says how "
                                f"many there are")
    return int(max_edges)


class RelationList:
    """A relation table over the entities of a graph, resident on the device: r rows (a, b) in any orientation, repeats and
    a == b allowed.  Nothing is normalised — a subgraph answers in row numbers of this table, where the caller keeps each
    relation's type and description.  A row with an end outside [0, n_entities) is part of no subgraph.
    pairs: an [r][2] integer array-like, uploaded once, or an int64 device tensor [r][2], used where it is.
    weights: one number per row, of any numeric type; only gathered for the rows an answer returns.
    types: one relation type per row, an integer in [0, 32) (type_ids() maps names to them), kept on the device as int32: a typed
    call (relation_types=) lists a row only for the queries whose filter holds its type."""

    @staticmethod
    def type_ids(names):
        """Type names -> (ids int32 [r], vocabulary): a name's id is its rank by first appearance, vocabulary[id] the name.
        RarcUnsupported for more than 32 distinct names."""
        vocabulary, index, ids = [], {}, []
        for name in names:
            if name not in index:
                if len(vocabulary) == MAX_TYPES:
                    raise B.RarcUnsupported(f"more than {MAX_TYPES} distinct relation types: an edge mask and a query filter hold {MAX_TYPES} "
                                            f"bits (the 33rd is {name!r})")
                index[name] = len(vocabulary)
                vocabulary.append(name)
            ids.append(index[name])
        return np.array(ids, np.int32), vocabulary

    def __init__(self, n_entities: int, pairs, weights=None, types=None, device: int = 0):
        import torch

        on_device = isinstance(pairs, torch.Tensor) and pairs.is_cuda
        if on_device:
            if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
                raise ValueError(f"expected an int64 [r][2] tensor of relations, got {pairs.dtype} {tuple(pairs.shape)}")
            r = int(pairs.shape[0])
        else:
            arr = np.asarray(pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
            if arr.ndim != 2 or arr.shape[1] != 2:
                raise ValueError(f"expected [r][2] relations, got an array of shape {arr.shape}")
            if not np.issubdtype(arr.dtype, np.integer):
                raise ValueError(f"relations must be integers, got {arr.dtype}")
            r = int(arr.shape[0])
        if r < 1:
            raise ValueError("a relation list needs at least 1 row")
        if r >= MAX_RELATIONS:
            raise B.RarcUnsupported(f"RelationList of {r} rows: the kernels take r < 2^31 - 1")
        w = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(weights)))
            if tuple(w.shape) != (r,) or w.dtype == torch.bool or w.is_complex():
                raise ValueError(f"expected {r} numeric weights, got {w.dtype} {tuple(w.shape)}")
        ty = None
        if types is not None:
            ty = check_type_ids(types.cpu().numpy() if isinstance(types, torch.Tensor) else types, r, "row")
        if not torch.cuda.is_available():
            raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
        self.n_entities, self.r = int(n_entities), r
        self.device = torch.device("cuda", device)
        if on_device and pairs.device != self.device:
            raise ValueError(f"the relations live on {pairs.device} and device={device} was asked for")
        with torch.cuda.device(self.device):
            self._pairs = pairs.contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64))).to(self.device)
            self._weights = None if w is None else w.to(self.device)
            self._types = None if ty is None else torch.from_numpy(ty).to(self.device)

    @property
    def typed(self) -> bool:
        return getattr(self, "_types", None) is not None

    def extended(self, rows, weights=None, types=None, n_entities=None):
        """A NEW RelationList over n_entities >= self.n_entities entities: this table's rows, then `rows` — existing rows keep
        their row numbers, so the caller's types and descriptions stay valid.  Concatenated on the device (graph_db/ingest.py).
        ValueError when the rows carry weights or types and this list does not, or the reverse."""
        from . import ingest

        return ingest.relations_extended(self, rows, weights=weights, types=types, n_entities=n_entities)


def check_relations(graph, relations, typed: bool = False):
    """ValueError for anything but None or a RelationList over the graph's vertices on the graph's device; typed: the call has
    relation_types, and the list must carry a type per row"""
    if relations is None:
        return
    if not isinstance(relations, RelationList):
        raise ValueError("relations must be a RelationList (or None for the graph's own pair list)")
    if typed and not relations.typed:
        raise ValueError("relation_types with a RelationList without types: build it with RelationList(..., types=), one type per row")
    if relations.n_entities != graph.n:
        raise ValueError(f"the relation list is over {relations.n_entities} entities and the graph has {graph.n} vertices: entity i must be "
                         f"vertex i")
    if relations.device != graph.device:
        raise ValueError(f"the relation list lives on {relations.device} and the graph on {graph.device}")


EDGE_FIELDS = ("edge_ids", "edge_ends", "edge_levels", "edge_counts", "edge_level_counts", "edge_weights")
SubgraphEdges = collections.namedtuple("SubgraphEdges", EDGE_FIELDS, defaults=(None,))
Subgraph = collections.namedtuple("Subgraph", ("vertex_ids", "vertex_hops", "vertex_counts", "hop_counts") + EDGE_FIELDS, defaults=(None,))


def _own_relations(graph):
    """the graph's own normalised pair list (every pair i < j, once) and its weights, as a RelationList that adopts them"""
    rel = getattr(graph, "_own_relation_list", None)
    if rel is None:
        w = graph._pair_weights
        w = None if w is None else w.to(graph.torch.int64) & 0xFFFFFFFF                      # (the uint32 weights, kept as their int32 bits)
        graph._own_relation_list = rel = RelationList(graph.n, graph._pairs, weights=w, device=graph.device.index)
    return rel


def _edges(graph, rel, nq, hops, max_edges, ws, wb, entry="rarc_khop_edges", filters=None):
    """the relations inside the neighbourhoods the traversal left in (ws, wb) -> device tensors, in the order of EDGE_FIELDS;
    entry="rarc_khop_path_edges": the relations on the paths of the path state in (ws, wb).  filters (device int32 [nq], uint32
    bits): the typed entry — a row needs its type in the query's filter; the graph's own pair list carries its masks instead"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    need = int(lib.rarc_khop_edges_workspace_bytes(rel.r, nq, hops))
    if need == 0:
        raise B.RarcError(f"neighbourhood_edges: {rel.r} relations, {nq} queries, hops={hops} refused by rarc_khop_edges_workspace_bytes")
    ews = getattr(graph, "_khop_ews", None)
    if ews is None or ews.numel() < need:
        graph._khop_ews = None
        graph._khop_ews = ews = t.empty(need, dtype=t.uint8, device=graph.device)
    ids = t.empty((nq, max_edges), dtype=t.int64, device=graph.device)
    lv = t.empty((nq, max_edges), dtype=t.int32, device=graph.device)
    cnt = t.empty(nq, dtype=t.int32, device=graph.device)
    lc = t.empty((nq, hops + 1), dtype=t.int32, device=graph.device)
    stream = t.cuda.current_stream(graph.device).cuda_stream
    if filters is None:
        B.check(getattr(lib, entry)(n, m, nq, hops, ws, wb, rel._pairs.data_ptr(), rel.r, max_edges, ews.data_ptr(), ews.numel(), ids.data_ptr(),
                                    lv.data_ptr(), cnt.data_ptr(), lc.data_ptr(), stream), entry)
    else:
        own = rel is getattr(graph, "_own_relation_list", None)
        row_types = graph._type_masks if own else rel._types
        B.check(getattr(lib, entry + "_typed")(n, m, nq, hops, ws, wb, rel._pairs.data_ptr(), rel.r, row_types.data_ptr(), int(own),
                                               filters.data_ptr(), max_edges, ews.data_ptr(), ews.numel(), ids.data_ptr(), lv.data_ptr(),
                                               cnt.data_ptr(), lc.data_ptr(), stream), entry + "_typed")
    rows = ids.clamp(min=0)                                                                  # the few returned rows: gathered here
    ends = t.where((ids >= 0).unsqueeze(-1), rel._pairs[rows], t.full_like(rel._pairs[:1], -1))
    out = (ids, ends, lv, cnt, lc)
    if rel._weights is not None:
        out += (t.where(ids >= 0, rel._weights[rows], t.zeros_like(rel._weights[:1])),)
    return out


def _subgraph(graph, rel, sd, hops, max_vertices, max_edges, early_stop, filters=None):
    """one launch batch, one traversal -> the vertex list (unless max_vertices is None) followed by the edge list"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    nq = int(sd.shape[0])
    ws, wb = traverse(graph, sd, hops, early_stop, filters)
    if max_vertices is None:
        return _edges(graph, rel, nq, hops, max_edges, ws, wb, filters=filters)
    ids = t.empty((nq, max_vertices), dtype=t.int64, device=graph.device)
    hp = t.empty((nq, max_vertices), dtype=t.int32, device=graph.device)
    cnt = t.empty(nq, dtype=t.int32, device=graph.device)
    hc = t.empty((nq, hops + 1), dtype=t.int32, device=graph.device)
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_list(n, m, nq, hops, max_vertices, ws, wb, ids.data_ptr(), hp.data_ptr(), cnt.data_ptr(), stream), "rarc_khop_list")
    B.check(lib.rarc_khop_counts(n, m, nq, hops, ws, wb, hc.data_ptr(), stream), "rarc_khop_counts")
    return (ids, hp, cnt, hc) + _edges(graph, rel, nq, hops, max_edges, ws, wb, filters=filters)


def neighbourhood_edges(graph, seeds, hops: int = 2, max_edges: int = 16384, relations=None, as_device: bool = False, early_stop: bool = False,
                        relation_types=None):
    hops, max_edges = check_hops(hops), check_max_edges(max_edges)
    filters = check_typed(graph, relation_types)
    check_relations(graph, relations, typed=filters is not None)
    with graph.torch.cuda.device(graph.device):
        rel = _own_relations(graph) if relations is None else relations
        sd = _device_seeds(graph, seeds)
        return SubgraphEdges(*_batched(graph, sd, as_device, lambda part, f: _subgraph(graph, rel, part, hops, None, max_edges, early_stop, f),
                                       filters))


def subgraph(graph, seeds, hops: int = 2, max_vertices: int = 4096, max_edges: int = 16384, relations=None, as_device: bool = False,
             early_stop: bool = False, relation_types=None):
    hops, max_edges = check_hops(hops, max_vertices), check_max_edges(max_edges)
    filters = check_typed(graph, relation_types)
    check_relations(graph, relations, typed=filters is not None)
    with graph.torch.cuda.device(graph.device):
        rel = _own_relations(graph) if relations is None else relations
        sd = _device_seeds(graph, seeds)
        return Subgraph(*_batched(graph, sd, as_device,
                                  lambda part, f: _subgraph(graph, rel, part, hops, int(max_vertices), max_edges, early_stop, f), filters))


def expand_subgraph(graph, index, queries, seeds_per_query: int = 5, hops: int = 2, max_vertices: int = 4096, max_edges: int = 16384,
                    relations=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
    hops, max_edges = check_hops(hops, max_vertices), check_max_edges(max_edges)
    filters = check_typed(graph, relation_types)
    check_relations(graph, relations, typed=filters is not None)
    graph._check_index(index, seeds_per_query)
    sd, _ = graph._index_seeds(index, queries, seeds_per_query)
    with graph.torch.cuda.device(graph.device):
        rel = _own_relations(graph) if relations is None else relations
        return Subgraph(*_batched(graph, sd, as_device,
                                  lambda part, f: _subgraph(graph, rel, part, hops, int(max_vertices), max_edges, early_stop, f), filters))


# ---- connecting paths: all shortest paths between sources (restated by tests/paths_ref.py) ------------------------------
MAX_PAIRS = 256                # pairs per call, and sources per call: one launch batch each
MAX_CONNECT_SEEDS = 23         # seeds_per_query of connect: 23 * 22 / 2 = 253 pairs of one query still fit one launch

PATH_FIELDS = ("distances", "vertex_ids", "vertex_positions", "vertex_counts", "position_counts") + EDGE_FIELDS
ShortestPaths = collections.namedtuple("ShortestPaths", PATH_FIELDS, defaults=(None,))
Connection = collections.namedtuple("Connection", PATH_FIELDS + ("pair_query", "pair_ends"), defaults=(None, None, None))


def paths_limits() -> dict:
    """The limits of rarc_khop_paths: the longest path looked for, and the sources and pairs of one call."""
    out = (ctypes.c_int * 3)()
    B.check(B.load_library().rarc_khop_paths_limits(out), "rarc_khop_paths_limits")
    return {"max_length": out[0], "max_sources": out[1], "max_pairs": out[2]}


def check_length(max_length) -> int:
    """ValueError for a negative max_length, RarcUnsupported, naming the limit, above 8"""
    if int(max_length) != max_length or int(max_length) < 0:
        raise ValueError(f"max_length must be an integer >= 0, got {max_length!r}")
    if int(max_length) > MAX_HOPS:
        raise B.RarcUnsupported(f"max_length={int(max_length)}: paths of at most {MAX_HOPS} edges are looked for (0 <= max_length <= {MAX_HOPS})")
    return int(max_length)


def check_path_caps(max_vertices, max_edges):
    """-> (max_vertices, max_edges) as integers; a path answer is always a list: ValueError below 1, RarcUnsupported above 65536"""
    if max_vertices is None:
        raise ValueError("max_vertices must be an integer >= 1: the vertices on the paths are returned as a list")
    if int(max_vertices) != max_vertices or int(max_vertices) < 1:
        raise ValueError(f"max_vertices must be an integer >= 1, got {max_vertices!r}")
    if int(max_vertices) > MAX_LIST_VERTICES:
        raise B.RarcUnsupported(f"max_vertices={int(max_vertices)}: a list holds at most 2^16 = {MAX_LIST_VERTICES} vertices; position_counts "
                                f"says how many lie on the paths")
    return int(max_vertices), check_max_edges(max_edges)


def host_sources(n: int, sources) -> np.ndarray:
    """host_seeds for the sources of a path query; RarcUnsupported for more than 256 of them"""
    sd = host_seeds(n, sources)
    if sd.shape[0] > MAX_PAIRS:
        raise B.RarcUnsupported(f"{sd.shape[0]} sources: one call takes at most {MAX_PAIRS}")
    return sd


def host_pairs(ns: int, pairs) -> np.ndarray:
    """[np][2] source indices -> int32 [np][2].  ValueError for no pairs, another shape, or an index outside [0, ns);
    RarcUnsupported for more than 256 pairs"""
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError(f"expected [np][2] pairs of source indices, np >= 1, got an array of shape {p.shape}")
    if p.shape[0] > MAX_PAIRS:
        raise B.RarcUnsupported(f"{p.shape[0]} pairs: one call takes at most {MAX_PAIRS}")
    if not np.all(p == np.floor(p)) or p.min() < 0 or p.max() >= ns:
        raise ValueError(f"a pair names a source outside [0, {ns})")
    return np.ascontiguousarray(p.astype(np.int32))


def _device_sources(graph, sources, pairs):
    """sources as neighbourhood takes seeds, pairs [np][2] -> (device int64 [ns][s], device int32 [np][2]), checked"""
    t = graph.torch
    if isinstance(sources, t.Tensor):
        sd = graph._seed_tensors(sources, None)[0]
        if int(sd.shape[0]) > MAX_PAIRS:
            raise B.RarcUnsupported(f"{int(sd.shape[0])} sources: one call takes at most {MAX_PAIRS}")
    else:
        sd = t.from_numpy(host_sources(graph.n, sources)).to(graph.device)
    ns = int(sd.shape[0])
    if isinstance(pairs, t.Tensor) and pairs.is_cuda:
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or pairs.dtype not in (t.int32, t.int64):
            raise ValueError(f"expected an int32 or int64 [np][2] tensor of pairs, np >= 1, got {pairs.dtype} {tuple(pairs.shape)}")
        if int(pairs.shape[0]) > MAX_PAIRS:
            raise B.RarcUnsupported(f"{int(pairs.shape[0])} pairs: one call takes at most {MAX_PAIRS}")
        if not bool(((pairs >= 0) & (pairs < ns)).all().item()):
            raise ValueError(f"a pair names a source outside [0, {ns})")
        return sd, pairs.to(device=graph.device, dtype=t.int32).contiguous()
    return sd, t.from_numpy(host_pairs(ns, pairs.cpu().numpy() if isinstance(pairs, t.Tensor) else pairs)).to(graph.device)


def mark_paths(graph, sd, pd, length: int, early_stop: bool = False, filters=None):
    """One traversal of the sources `sd` to `length`, then rarc_khop_paths for the pairs `pd` -> (distances, a device int32
    [np]; path workspace pointer, bytes): a k-hop state of np columns with positions for hops, for the k-hop readers.
    filters: None, or the one filter of a typed call as host uint32 [1]: every source traverses under it"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    ns, npairs = int(sd.shape[0]), int(pd.shape[0])
    ws, wb = traverse(graph, sd, length, early_stop, _device_filters(graph, filters, ns))
    need = int(lib.rarc_khop_workspace_bytes(n, m, npairs, length))
    if need == 0:
        raise B.RarcError(f"shortest_paths: n={n}, m={m}, {npairs} pairs, max_length={length} refused by rarc_khop_workspace_bytes")
    pws = getattr(graph, "_path_ws", None)
    if pws is None or pws.numel() < need:
        graph._path_ws = None
        graph._path_ws = pws = t.empty(need, dtype=t.uint8, device=graph.device)
    dist = t.empty(npairs, dtype=t.int32, device=graph.device)
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_paths(n, m, ns, npairs, length, ws, wb, pd.data_ptr(), pws.data_ptr(), pws.numel(), dist.data_ptr(), stream),
            "rarc_khop_paths")
    return dist, pws.data_ptr(), pws.numel()


def _paths(graph, rel, sd, pd, length, max_vertices, max_edges, early_stop, filters=None):
    """one call -> device tensors in the order of PATH_FIELDS"""
    t, lib, n, m = graph.torch, graph.lib, graph.n, graph.m
    npairs = int(pd.shape[0])
    dist, pws, pwb = mark_paths(graph, sd, pd, length, early_stop, filters)
    ids = t.empty((npairs, max_vertices), dtype=t.int64, device=graph.device)
    pos = t.empty((npairs, max_vertices), dtype=t.int32, device=graph.device)
    cnt = t.empty(npairs, dtype=t.int32, device=graph.device)
    pc = t.empty((npairs, length + 1), dtype=t.int32, device=graph.device)
    stream = t.cuda.current_stream(graph.device).cuda_stream
    B.check(lib.rarc_khop_list(n, m, npairs, length, max_vertices, pws, pwb, ids.data_ptr(), pos.data_ptr(), cnt.data_ptr(), stream), "rarc_khop_list")
    B.check(lib.rarc_khop_counts(n, m, npairs, length, pws, pwb, pc.data_ptr(), stream), "rarc_khop_counts")
    return (dist, ids, pos, cnt, pc) + _edges(graph, rel, npairs, length, max_edges, pws, pwb, entry="rarc_khop_path_edges",
                                              filters=_device_filters(graph, filters, npairs))


def _host(out, as_device):
    return out if as_device else tuple(x.cpu().numpy() for x in out)


def shortest_paths(graph, sources, pairs, max_length: int = 4, max_vertices: int = 4096, max_edges: int = 16384, relations=None,
                   as_device: bool = False, early_stop: bool = False, relation_types=None):
    length = check_length(max_length)
    max_vertices, max_edges = check_path_caps(max_vertices, max_edges)
    filters = _single_filter(graph, relation_types)
    check_relations(graph, relations, typed=filters is not None)
    with graph.torch.cuda.device(graph.device):
        sd, pd = _device_sources(graph, sources, pairs)
        rel = _own_relations(graph) if relations is None else relations
        return ShortestPaths(*_host(_paths(graph, rel, sd, pd, length, max_vertices, max_edges, early_stop, filters), as_device))


def path_chunks(graph, mentions, sources, pairs, max_length: int = 4, decay=None, top_k=None, as_device: bool = False,
                early_stop: bool = False, relation_types=None):
    length = check_length(max_length)
    decay = check_decay(decay, length)
    filters = _single_filter(graph, relation_types)
    _check_mentions(graph, mentions, top_k)
    t, lib = graph.torch, graph.lib
    with t.cuda.device(graph.device):
        sd, pd = _device_sources(graph, sources, pairs)
        npairs = int(pd.shape[0])
        _, pws, pwb = mark_paths(graph, sd, pd, length, early_stop, filters)
        cws, cb = mentions.workspace(npairs)
        split, n_split = mentions.split_list()
        stream = t.cuda.current_stream(graph.device).cuda_stream
        B.check(lib.rarc_khop_chunks(graph.n, graph.m, npairs, length, decay.ctypes.data, pws, pwb, mentions._row_ptr.data_ptr(),
                                     mentions._ent.data_ptr(), mentions._w.data_ptr(), mentions.n_chunks, mentions.nnz, split, n_split, cws, cb,
                                     stream), "rarc_khop_chunks")
        out = mentions.ranked(npairs, None if top_k is None else int(top_k))
        out = _host((out,) if top_k is None else out, as_device)
        return out[0] if top_k is None else tuple(out)


def connect(graph, index, queries, seeds_per_query: int = 5, max_length: int = 4, max_vertices: int = 4096, max_edges: int = 16384,
            relations=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
    length = check_length(max_length)
    max_vertices, max_edges = check_path_caps(max_vertices, max_edges)
    filters = _single_filter(graph, relation_types)
    check_relations(graph, relations, typed=filters is not None)
    graph._check_index(index, seeds_per_query)
    k = int(seeds_per_query)
    if k < 2:
        raise ValueError("connect pairs the seeds of a query: seeds_per_query must be at least 2")
    if k > MAX_CONNECT_SEEDS:
        raise B.RarcUnsupported(f"seeds_per_query={k}: the {k * (k - 1) // 2} pairs of one query exceed the {MAX_PAIRS} of one launch "
                                f"(seeds_per_query <= {MAX_CONNECT_SEEDS})")
    t = graph.torch
    ids, _ = graph._index_seeds(index, queries, k)                                           # int64 [Q][k], on the device
    i, j = np.triu_indices(k, 1)
    per_query = np.stack([i, j], axis=1).astype(np.int32)                                    # every i < j of one query's seeds
    step = min(MAX_PAIRS // k, MAX_PAIRS // len(per_query))                                  # queries per launch batch
    with t.cuda.device(graph.device):
        rel = _own_relations(graph) if relations is None else relations
        parts = []
        for q0 in range(0, int(ids.shape[0]), step):
            part = ids[q0:q0 + step]
            nq = int(part.shape[0])
            local = (per_query[None] + (np.arange(nq, dtype=np.int32) * k)[:, None, None]).reshape(-1, 2)
            pd = t.from_numpy(local).to(graph.device)
            sd = part.reshape(-1, 1).contiguous()                                            # every seed a one-vertex source
            pq = t.from_numpy(np.repeat(np.arange(q0, q0 + nq, dtype=np.int32), len(per_query))).to(graph.device)
            ends = sd[:, 0][pd.to(t.int64)]
            parts.append(_paths(graph, rel, sd, pd, length, max_vertices, max_edges, early_stop, filters) + (pq, ends))
        if rel._weights is None:                                                             # edge_weights stays None, before the two pair fields
            parts = [p[:-2] + (None,) + p[-2:] for p in parts]
        out = tuple(None if p0 is None else (p0 if len(parts) == 1 else t.cat([p[f] for p in parts])) for f, p0 in enumerate(parts[0]))
        return Connection(*(out if as_device else tuple(None if x is None else x.cpu().numpy() for x in out)))


def _check_one_shot_types(types, kw, nq=None, single=False):
    """the typed arguments of a one-shot form, before the graph is built: relation_types needs `types` (one id per pair), its
    ids must lie in [0, 32) and its filters number 1 or nq (paths: 1)"""
    if kw.get("relation_types") is None:
        return
    if types is None:
        raise ValueError("relation_types on a graph without type masks: give types=, one relation type per pair")
    filters = host_filters(kw["relation_types"])
    if single and filters.shape[0] != 1:
        raise ValueError(f"{filters.shape[0]} filters on a paths call: give one iterable of type ids")
    if nq is not None:
        spread_filters(filters, nq)


def all_shortest_paths(n: int, edges, sources, pairs, device: int = 0, types=None, **kw):
    """The one-shot form: EntityGraph(n, edges, types=types, device=device).shortest_paths(sources, pairs, **kw).  The arguments
    are checked before the graph is built: a bad source, pair, max_length, max_vertices, max_edges, relation list or filter raises
    with no device visible."""
    from .pagerank import EntityGraph

    _check_one_shot_types(types, kw, single=True)

    check_length(kw.get("max_length", 4))
    check_path_caps(kw.get("max_vertices", 4096), kw.get("max_edges", 16384))
    rel = kw.get("relations")
    if rel is not None and (not isinstance(rel, RelationList) or rel.n_entities != int(n)):
        raise ValueError(f"relations must be a RelationList over the graph's {int(n)} vertices (or None for the graph's own pair list)")
    if not hasattr(sources, "is_cuda"):
        ns = host_sources(int(n), sources).shape[0]
        if not hasattr(pairs, "is_cuda"):
            host_pairs(ns, pairs)
    return EntityGraph(n, edges, types=types, device=device).shortest_paths(sources, pairs, **kw)


def k_hop_subgraph(n: int, pairs, seeds, hops: int = 2, device: int = 0, types=None, **kw):
    """The one-shot form: EntityGraph(n, pairs, types=types, device=device).subgraph(seeds, hops, **kw).  The arguments are checked
    before the graph is built: a bad seed, hops, max_vertices, max_edges, relation list or filter raises with no device visible."""
    from .pagerank import EntityGraph

    _check_one_shot_types(types, kw, None if hasattr(seeds, "is_cuda") else len(list(seeds)))

    check_hops(hops, kw.get("max_vertices", 4096))
    check_max_edges(kw.get("max_edges", 16384))
    rel = kw.get("relations")
    if rel is not None and (not isinstance(rel, RelationList) or rel.n_entities != int(n)):
        raise ValueError(f"relations must be a RelationList over the graph's {int(n)} vertices (or None for the graph's own pair list)")
    if not hasattr(seeds, "is_cuda"):
        host_seeds(int(n), seeds)
    return EntityGraph(n, pairs, types=types, device=device).subgraph(seeds, hops=hops, **kw)


def k_hop(n: int, pairs, seeds, hops: int = 2, device: int = 0, types=None, **kw):
    """The one-shot form: EntityGraph(n, pairs, types=types, device=device).neighbourhood(seeds, hops, **kw).  The arguments are
    checked before the graph is built: a bad seed, hops, max_vertices or filter raises with no device visible."""
    from .pagerank import EntityGraph

    _check_one_shot_types(types, kw, None if hasattr(seeds, "is_cuda") else len(list(seeds)))

    check_hops(hops, kw.get("max_vertices"))
    if not hasattr(seeds, "is_cuda"):
        host_seeds(int(n), seeds)
    return EntityGraph(n, pairs, types=types, device=device).neighbourhood(seeds, hops=hops, **kw)
