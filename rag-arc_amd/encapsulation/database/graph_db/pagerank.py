"""Personalized PageRank over the entity graph, on the MI355X (csrc/ppr.hip): the retrieval a graph store is queried with.

What it replaces: the reference stores entities, events and their relations and leaves every graph computation to Neo4j GDS;
a retriever over that graph (HippoRAG-style, or upstream RAG-ARC's graph retriever) runs

    CALL gds.pageRank.stream(graph, {sourceNodes: seeds, dampingFactor: 0.85, maxIterations: 20})

once per query.  Here a batch of queries is one sparse-matrix x dense-matrix power iteration next to the CSR `rarc_graph_csr`
built: `EntityGraph(n, pairs)` keeps the graph resident, `personalized_pagerank(seeds)` ranks from given seeds, and
`retrieve(index, queries)` takes the seeds from a `FlatIndexF16` search without leaving HBM.

The rule is fixed point (restated by tests/ppr_ref.py): the scores are the same bits for any order of the
edges and any batch, and row q of a batch equals the one-query call.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import ctypes

import numpy as np

from ....hip import binding as B
from .communities import MAX_EDGES, MAX_VERTICES

ONE = 1 << 40                  # the unit of mass (csrc/ppr.hip)
MAX_SEEDS = 64                 # seed slots per query
MAX_SEED_WEIGHT = 1 << 20      # a seed weight after quantisation
MAX_BATCH = 256                # queries per launch; larger batches are cut here
MAX_TOP_K = 8192
MAX_TOPK_VERTICES = 1 << 24    # the top-k key carries the vertex in 24 bits
MAX_TOTAL_WEIGHT = 1 << 31     # total edge weight: every weighted degree then fits 32 bits


def limits() -> dict:
    """The shape limits of the kernels (csrc/ppr.hip): the largest degree one wave walks (a vertex of a larger one is split
    across a workgroup), the largest batch of the vertex-parallel form of the step, and the argument limits."""
    out = (ctypes.c_int * 6)()
    B.check(B.load_library().rarc_ppr_limits(out), "rarc_ppr_limits")
    return {"split_degree": out[0], "vertex_parallel_max_batch": out[1], "max_batch": out[2], "max_seeds": out[3], "max_top_k": out[4],
            "topk_vertex_bits": out[5]}


def quantise_seed_weights(w: np.ndarray) -> np.ndarray:
    """float [B][s] >= 0 -> uint32: each row scaled so its largest weight is 1, then round(w * 2^20); an all-zero row stays zero"""
    w = np.asarray(w, dtype=np.float64)
    mx = w.max(axis=1, keepdims=True) if w.shape[1] else np.zeros((w.shape[0], 1))
    safe = np.where(mx > 0, mx, 1.0)
    return np.rint(w / safe * float(MAX_SEED_WEIGHT)).astype(np.uint32)


def _normalise_pairs(n: int, pairs, weights):
    """exactly louvain_communities' normalisation of host pairs (swapped to i < j, duplicates dropped); the weights of
    duplicates add up"""
    return _normalise_typed_pairs(n, pairs, weights, None)[:2]


def _normalise_typed_pairs(n: int, pairs, weights, types):
    """_normalise_pairs with one relation type per input pair (or None) -> (pairs, weights, masks): the uint32 mask of a pair is
    the OR of 1 << type over its duplicates, in either orientation"""
    from .neighbourhood import check_type_ids

    arr = np.asarray(pairs)
    if arr.size == 0:
        arr = np.zeros((0, 2), np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError(f"expected [m][2] pairs, got an array of shape {arr.shape}")
    if not np.issubdtype(arr.dtype, np.integer):
        if not np.all(arr == np.floor(arr)):
            raise ValueError("pairs must be integers")
    arr = arr.astype(np.int64)
    w = None
    if weights is not None:
        w = np.asarray(weights)
        if w.shape != (arr.shape[0],):
            raise ValueError(f"expected {arr.shape[0]} weights, got an array of shape {w.shape}")
        if not np.all(w == np.floor(w)) or (w.size and (w.min() < 1 or w.max() >= 1 << 32)):
            raise ValueError("edge weights must be integers in [1, 2^32)")
        w = w.astype(np.int64)
    masks = None
    if types is not None:
        masks = np.uint32(1) << check_type_ids(types, arr.shape[0], "pair").astype(np.uint32)
    if arr.shape[0]:
        if arr.min() < 0 or arr.max() >= n:
            raise ValueError(f"a pair names a vertex outside [0, {n})")
        if np.any(arr[:, 0] == arr[:, 1]):
            raise ValueError("a pair (i, i): self-loops are not part of the input")
        arr, inverse = np.unique(np.stack([arr.min(axis=1), arr.max(axis=1)], axis=1), axis=0, return_inverse=True)
        if w is not None:
            w = np.bincount(inverse.ravel(), weights=w.astype(np.float64), minlength=arr.shape[0]).astype(np.int64)
        if masks is not None:
            joined = np.zeros(arr.shape[0], np.uint32)
            np.bitwise_or.at(joined, inverse.ravel(), masks)
            masks = joined
    return arr, w, masks


class EntityGraph:
    """An undirected graph on n vertices, resident on the device as the CSR of `rarc_graph_csr`.
    pairs: an [m][2] array-like — normalised as louvain_communities normalises it: swapped to i < j, duplicates dropped (the
    weights of duplicates add up) — or an int64 device tensor [m][2], used where it is: every pair i < j, each once.
    weights: integers >= 1 per pair (unit by default), their total below 2^31.
    types: one relation type per input pair, an integer in [0, 32) (RelationList.type_ids maps names to them): the graph keeps a
    uint32 mask per edge, the OR over its duplicates, and the query calls take relation_types=."""

    def __init__(self, n: int, pairs, weights=None, types=None, device: int = 0):
        import torch

        n = int(n)
        on_device = isinstance(pairs, torch.Tensor) and pairs.is_cuda
        masks = None
        if on_device:
            if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
                raise ValueError(f"expected an int64 [m][2] tensor of pairs, got {pairs.dtype} {tuple(pairs.shape)}")
            m = int(pairs.shape[0])
            w = None
            if weights is not None:
                w = np.asarray(weights.cpu().numpy() if isinstance(weights, torch.Tensor) else weights)
                if w.shape != (m,) or not np.all(w == np.floor(w)) or (m and (w.min() < 1 or w.max() >= 1 << 32)):
                    raise ValueError(f"edge weights must be {m} integers in [1, 2^32)")
                w = w.astype(np.int64)
            if types is not None:                                       # (device pairs are unique by contract: a pair's mask is its one type)
                from .neighbourhood import check_type_ids

                masks = np.uint32(1) << check_type_ids(types.cpu().numpy() if isinstance(types, torch.Tensor) else types, m, "pair").astype(np.uint32)
        else:
            arr, w, masks = _normalise_typed_pairs(n, pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs, weights, types)
            m = int(arr.shape[0])
        if n < 2:
            raise ValueError("a graph needs at least 2 vertices")
        if m < 1:
            raise ValueError("a graph needs at least 1 edge")
        if m >= MAX_EDGES or n >= MAX_VERTICES:
            raise B.RarcUnsupported(f"EntityGraph(n={n}, {m} edges): the kernels take n < 2^31 - 1 vertices and m < 2^30 edges")
        if (int(w.sum()) if w is not None else m) >= MAX_TOTAL_WEIGHT:
            raise B.RarcUnsupported("the total edge weight must stay below 2^31 (every weighted degree then fits 32 bits)")
        if on_device and not bool(((pairs[:, 0] >= 0) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < n)).all().item()):
            raise ValueError(f"device pairs must satisfy 0 <= i < j < {n}")
        if not torch.cuda.is_available():
            raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
        self.torch, self.lib = torch, B.load_library()
        self.n, self.m = n, m
        self.device = torch.device("cuda", device)
        with torch.cuda.device(self.device):
            p = pairs.to(self.device).contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
            wd = None if w is None else torch.from_numpy(w.astype(np.uint32).view(np.int32)).to(self.device)
            self._graph = torch.empty(int(self.lib.rarc_graph_csr_workspace_bytes(n, m)), dtype=torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            B.check(self.lib.rarc_graph_csr(p.data_ptr(), wd.data_ptr() if wd is not None else None, None, n, m, self._graph.data_ptr(),
                                            self._graph.numel(), stream), "rarc_graph_csr")
            torch.cuda.current_stream(self.device).synchronize()
            md = None if masks is None else torch.from_numpy(masks.view(np.int32)).to(self.device)
        self._pairs, self._pair_weights = p, wd                         # kept for subgraph(relations=None): 16 bytes an edge
        self._type_masks, self._typed_adj = md, None                    # uint32 bits [m]; the typed slot arrays, built on the first typed call
        self._ws = None
        self._components = {}                                           # as_device -> Components, filled by components()

    @property
    def typed(self) -> bool:
        """whether the edges carry type masks: relation_types= is refused without them"""
        return getattr(self, "_type_masks", None) is not None

    @classmethod
    def from_relations(cls, relations, device=None):
        """The graph of a typed RelationList: every row (a, b, t) with a != b and both ends in [0, n_entities) is a relation of
        the pair {a, b}; the pair's mask is the OR of 1 << t over its rows, its weight the number of its rows or, where the list
        has weights, their sum (integers >= 1, as the constructor takes them)."""
        from .neighbourhood import RelationList

        if not isinstance(relations, RelationList) or not relations.typed:
            raise ValueError("from_relations takes a RelationList with types")
        n = relations.n_entities
        p = relations._pairs.cpu().numpy()
        keep = (p[:, 0] != p[:, 1]) & (p >= 0).all(axis=1) & (p < n).all(axis=1)
        w = None if relations._weights is None else relations._weights.cpu().numpy()[keep]
        return cls(n, p[keep], weights=np.ones(int(keep.sum()), np.int64) if w is None else w, types=relations._types.cpu().numpy()[keep],
                   device=relations.device.index if device is None else device)

    @classmethod
    def from_device(cls, n: int, pairs, weights=None, type_masks=None):
        """Adopts buffers that are on a device already (graph_db/merge.py builds a merged graph this way): `pairs` an int64 device
        tensor [m][2], every pair 0 <= i < j < n, each once, and `weights` None (unit) or a device tensor [m] of int32 holding
        uint32 bits (what rarc_merge_pairs writes), each >= 1; `type_masks` None or a device tensor [m] of int32 holding each pair's
        uint32 mask of relation types.  Nothing passes through the host but the two words of the checks:
        the same limits as the constructor's, refused the same way."""
        import torch

        n = int(n)
        if not (isinstance(pairs, torch.Tensor) and pairs.is_cuda and pairs.ndim == 2 and pairs.shape[1] == 2 and pairs.dtype == torch.int64):
            raise ValueError("expected an int64 [m][2] device tensor of pairs")
        m = int(pairs.shape[0])
        if weights is not None and not (isinstance(weights, torch.Tensor) and weights.device == pairs.device and weights.dtype == torch.int32
                                        and tuple(weights.shape) == (m,)):
            raise ValueError(f"edge weights must be an int32 device tensor [{m}] (uint32 bits) beside the pairs")
        if type_masks is not None and not (isinstance(type_masks, torch.Tensor) and type_masks.device == pairs.device
                                           and type_masks.dtype == torch.int32 and tuple(type_masks.shape) == (m,)):
            raise ValueError(f"type masks must be an int32 device tensor [{m}] (uint32 bits) beside the pairs")
        if n < 2:
            raise ValueError("a graph needs at least 2 vertices")
        if m < 1:
            raise ValueError("a graph needs at least 1 edge")
        if m >= MAX_EDGES or n >= MAX_VERTICES:
            raise B.RarcUnsupported(f"EntityGraph(n={n}, {m} edges): the kernels take n < 2^31 - 1 vertices and m < 2^30 edges")
        self = cls.__new__(cls)
        self.torch, self.lib = torch, B.load_library()
        self.n, self.m = n, m
        self.device = pairs.device
        with torch.cuda.device(self.device):
            p = pairs.contiguous()
            wd = None if weights is None else weights.contiguous()
            ok = ((p[:, 0] >= 0) & (p[:, 0] < p[:, 1]) & (p[:, 1] < n)).all()
            total = torch.tensor(m, device=self.device) if wd is None else (wd.to(torch.int64) & 0xFFFFFFFF).sum()
            least = torch.tensor(1, device=self.device) if wd is None else (wd.to(torch.int64) & 0xFFFFFFFF).min()
            ok, total, least = torch.stack([ok.to(torch.int64), total, least]).tolist()
            if not ok:
                raise ValueError(f"device pairs must satisfy 0 <= i < j < {n}")
            if least < 1:
                raise ValueError("edge weights must be integers in [1, 2^32)")
            if total >= MAX_TOTAL_WEIGHT:
                raise B.RarcUnsupported("the total edge weight must stay below 2^31 (every weighted degree then fits 32 bits)")
            self._graph = torch.empty(int(self.lib.rarc_graph_csr_workspace_bytes(n, m)), dtype=torch.uint8, device=self.device)
            stream = torch.cuda.current_stream(self.device).cuda_stream
            B.check(self.lib.rarc_graph_csr(p.data_ptr(), wd.data_ptr() if wd is not None else None, None, n, m, self._graph.data_ptr(),
                                            self._graph.numel(), stream), "rarc_graph_csr")
            torch.cuda.current_stream(self.device).synchronize()
        self._pairs, self._pair_weights = p, wd
        self._type_masks, self._typed_adj = None if type_masks is None else type_masks.contiguous(), None
        self._ws = None
        self._components = {}
        return self

    @classmethod
    def from_rows(cls, n: int, rows, weights=None, types=None, device: int = 0, on_invalid: str = "raise"):
        """The graph of raw extraction rows, normalised on the device (graph_db/ingest.py): `rows` a host array-like
        or an int64 device tensor [r][2], in any orientation, with duplicates; `weights` integers per row (host, or a device int32
        tensor of uint32 bits), unit by default; `types` one relation type per row (host, or a device int32 tensor).  Nothing is
        normalised on the host; the result equals EntityGraph(n, rows, weights, types) where that takes the rows.
        A row with an end outside [0, n), a == b, weight 0 or a type outside [0, 32) is no edge: on_invalid="raise" raises
        ValueError naming the kinds and counts, "skip" leaves such rows out and reports {kind: count} as `.skipped`.
        Refused as the constructor refuses: no edge at all (ValueError); a summed edge weight >= 2^32, a total >= 2^31, or
        2^31 rows and more (RarcUnsupported)."""
        from . import ingest

        return ingest.graph_from_rows(cls, n, rows, weights=weights, types=types, device=device, on_invalid=on_invalid)

    def extended(self, rows, weights=None, types=None, n=None, on_invalid: str = "raise"):
        """A NEW EntityGraph over n >= self.n vertices (default: as many): this graph's edges and `rows`, as from_rows takes them,
        folded together on the device — equal to the constructor on this graph's rows followed by the new ones.  This graph is not
        modified, so calls in flight on it are unaffected.  When only one side carries weights the other side's rows count 1
        each.  ValueError, before any launch, for n < self.n, or when the graph carries types and the rows do not or the reverse."""
        from . import ingest

        return ingest.graph_from_rows(type(self), self.n if n is None else n, rows, weights=weights, types=types, on_invalid=on_invalid, base=self)

    # ---------------------------------------------------------------------------------------------------------------- arguments
    @staticmethod
    def _check_run(damping, max_iterations, tolerance, top_k, n):
        damping, tolerance = float(damping), float(tolerance)
        if not 0.0 <= damping < 1.0:
            raise ValueError("damping must lie in [0, 1)")
        a = int(round(damping * 65536))
        if a >= 65536:
            raise ValueError("damping rounds to 1 at 16 bits")
        if int(max_iterations) < 0:
            raise ValueError("max_iterations must not be negative")
        if not 0.0 <= tolerance <= 1.0:
            raise ValueError("tolerance must lie in [0, 1]")
        if top_k is not None:
            if not 1 <= int(top_k) <= MAX_TOP_K:
                raise ValueError(f"top_k must lie in [1, {MAX_TOP_K}]")
            if n >= MAX_TOPK_VERTICES:
                raise B.RarcUnsupported(f"top_k over n={n} vertices: the top-k key carries the vertex in 24 bits, n < 2^24 = "
                                        f"{MAX_TOPK_VERTICES}; ask for the scores (top_k=None) instead")
        return a, int(tolerance * ONE)

    def _seed_tensors(self, seeds, seed_weights):
        """-> (device int64 [B][s], device int32 [B][s] holding the uint32 weights)"""
        t = self.torch
        if isinstance(seeds, t.Tensor):
            if seeds.ndim != 2 or seeds.dtype != t.int64:
                raise ValueError(f"expected an int64 [B][s] tensor of seeds, got {seeds.dtype} {tuple(seeds.shape)}")
            nq, s = int(seeds.shape[0]), int(seeds.shape[1])
            if nq < 1:
                raise ValueError("no queries")
            if not 1 <= s <= MAX_SEEDS:
                raise ValueError(f"{s} seed slots per query: 1 .. {MAX_SEEDS} are taken")
            sd = seeds.to(self.device).contiguous()
            if not bool(((sd >= -1) & (sd < self.n)).all().item()):
                raise ValueError(f"a seed names a vertex outside [0, {self.n})")
            if seed_weights is None:
                wd = t.ones((nq, s), dtype=t.int32, device=self.device)
            elif isinstance(seed_weights, t.Tensor) and not seed_weights.dtype.is_floating_point:
                wd = seed_weights.to(self.device)
                if tuple(wd.shape) != (nq, s) or not bool(((wd >= 0) & (wd <= MAX_SEED_WEIGHT)).all().item()):
                    raise ValueError(f"integer seed weights must be [B][s] in [0, 2^20]")
                wd = wd.to(t.int32).contiguous()
            else:
                wf = t.as_tensor(seed_weights).to(device=self.device, dtype=t.float64)
                if tuple(wf.shape) != (nq, s) or not bool((t.isfinite(wf) & (wf >= 0)).all().item()):
                    raise ValueError("seed weights must be [B][s], finite and not negative")
                mx = wf.max(dim=1, keepdim=True).values
                wd = t.round(wf / t.where(mx > 0, mx, t.ones_like(mx)) * float(MAX_SEED_WEIGHT)).to(t.int32).contiguous()
            return sd, wd
        rows = [list(r) for r in seeds]
        if not rows:
            raise ValueError("no queries")
        s = max(1, max(len(r) for r in rows))
        if s > MAX_SEEDS:
            raise ValueError(f"{s} seeds in a query: at most {MAX_SEEDS} are taken")
        sd = np.full((len(rows), s), -1, np.int64)
        wf = np.zeros((len(rows), s), np.float64)
        for i, r in enumerate(rows):
            v = np.asarray(r)
            if v.size and (not np.all(v == np.floor(v)) or v.min() < 0 or v.max() >= self.n):
                raise ValueError(f"a seed names a vertex outside [0, {self.n})")
            sd[i, :len(r)] = v
            if seed_weights is None:
                wf[i, :len(r)] = 1.0
            else:
                w = np.asarray(seed_weights[i], dtype=np.float64)
                if w.shape != (len(r),):
                    raise ValueError(f"query {i}: {len(r)} seeds and weights of shape {w.shape}")
                if not np.all(np.isfinite(w)) or np.any(w < 0):
                    raise ValueError("seed weights must be finite and not negative")
                wf[i, :len(r)] = w
        wq = quantise_seed_weights(wf)
        return t.from_numpy(sd).to(self.device), t.from_numpy(wq.view(np.int32)).to(self.device)

    # ---------------------------------------------------------------------------------------------------------------- the run
    def _typed_filters(self, relation_types, seeds=None):
        """relation_types as the query calls take it -> None (the untyped run), or host uint32 filters; checked as the traversal
        calls check theirs, before anything is uploaded.  seeds: where the batch is known here, the filter count is checked too"""
        from . import neighbourhood as K

        filters = K.check_typed(self, relation_types)
        if filters is not None and seeds is not None:
            K.spread_filters(filters, int(seeds.shape[0]) if hasattr(seeds, "shape") else len(seeds))
        return filters

    def _iterate(self, sd, wd, a: int, tol: int, max_iterations: int, filters=None) -> int:
        """seeds one launch batch (<= 256 queries) and runs its steps in the workspace -> `cur`, as the next step would get it.
        filters: None, or a device int32 [nq] of uint32 filters — the typed seed and step over the weighted typed adjacency"""
        t, lib, n, m = self.torch, self.lib, self.n, self.m
        nq, s = int(sd.shape[0]), int(sd.shape[1])
        need = int(lib.rarc_ppr_workspace_bytes(n, m, nq))
        if need == 0:
            raise B.RarcError(f"personalized_pagerank: n={n}, m={m}, {nq} queries refused by rarc_ppr_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = t.empty(need, dtype=t.uint8, device=self.device)
        g, gb, ws, wb = self._graph.data_ptr(), self._graph.numel(), self._ws.data_ptr(), self._ws.numel()
        stream = t.cuda.current_stream(self.device).cuda_stream
        if filters is not None:
            from .neighbourhood import typed_adjacency

            ta = typed_adjacency(self, weighted=True)
            ty, tb, fd = ta.data_ptr(), ta.numel(), filters.data_ptr()
            B.check(lib.rarc_ppr_seed_typed(g, gb, ty, tb, fd, n, m, sd.data_ptr(), wd.data_ptr(), nq, s, ws, wb, stream), "rarc_ppr_seed_typed")
        else:
            B.check(lib.rarc_ppr_seed(g, gb, n, m, sd.data_ptr(), wd.data_ptr(), nq, s, ws, wb, stream), "rarc_ppr_seed")
        done = t.zeros(nq, dtype=t.int32, device=self.device) if tol > 0 else None
        cur = 0
        for _ in range(max_iterations):
            if filters is not None:
                B.check(lib.rarc_ppr_step_typed(g, gb, ty, tb, fd, n, m, nq, a, tol, cur, ws, wb, done.data_ptr() if done is not None else None,
                                                stream), "rarc_ppr_step_typed")
            else:
                B.check(lib.rarc_ppr_step(g, gb, n, m, nq, a, tol, cur, ws, wb, done.data_ptr() if done is not None else None, stream),
                        "rarc_ppr_step")
            cur ^= 1
            if done is not None and bool(done.all().item()):        # B words per iteration, only under a tolerance
                break
        return cur

    def _run(self, sd, wd, a: int, tol: int, max_iterations: int, top_k, mentions=None, filters=None):
        """one launch batch (<= 256 queries) -> device tensors: scores [B][n], or (ids, scores, counts); with `mentions` (a
        MentionMap) the same over its chunks: the iterations are shared, only the tail differs"""
        t, lib, n, m = self.torch, self.lib, self.n, self.m
        nq = int(sd.shape[0])
        cur = self._iterate(sd, wd, a, tol, max_iterations, filters)
        if mentions is not None:
            return mentions.project(n, m, nq, cur, self._ws, top_k)
        ws, wb = self._ws.data_ptr(), self._ws.numel()
        stream = t.cuda.current_stream(self.device).cuda_stream
        if top_k is None:
            out = t.empty((nq, n), dtype=t.float64, device=self.device)
            B.check(lib.rarc_ppr_scores(n, m, nq, ws, wb, out.data_ptr(), stream), "rarc_ppr_scores")
            return out
        ids = t.empty((nq, top_k), dtype=t.int64, device=self.device)
        sc = t.empty((nq, top_k), dtype=t.float64, device=self.device)
        cnt = t.empty(nq, dtype=t.int32, device=self.device)
        B.check(lib.rarc_ppr_topk(n, m, nq, top_k, cur, ws, wb, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stream), "rarc_ppr_topk")
        return ids, sc, cnt

    def _ranked(self, sd, wd, a, tol, max_iterations, top_k, as_device, mentions=None, filters=None):
        """cuts the queries at 256 per launch batch, and the host `filters` (None: untyped) with them"""
        t = self.torch
        more = {} if mentions is None else {"mentions": mentions}
        fd = None
        if filters is not None:
            from .neighbourhood import _device_filters

            fd = _device_filters(self, filters, int(sd.shape[0]))
        parts = [self._run(sd[s0:s0 + MAX_BATCH], wd[s0:s0 + MAX_BATCH], a, tol, int(max_iterations), top_k,
                           **(more if fd is None else {**more, "filters": fd[s0:s0 + MAX_BATCH]}))
                 for s0 in range(0, int(sd.shape[0]), MAX_BATCH)]
        if top_k is None:
            out = parts[0] if len(parts) == 1 else t.cat(parts)
            return out if as_device else out.cpu().numpy()
        out = parts[0] if len(parts) == 1 else tuple(t.cat([p[i] for p in parts]) for i in range(3))
        return out if as_device else tuple(x.cpu().numpy() for x in out)

    def personalized_pagerank(self, seeds, seed_weights=None, damping: float = 0.85, max_iterations: int = 20, tolerance: float = 0.0,
                              top_k=None, as_device: bool = False, relation_types=None):
        """Personalized PageRank from each query's seeds.
        seeds: a list of lists of vertices, or a device int64 [B][s] tensor padded with -1; at most 64 per query, a vertex may
        repeat.  seed_weights: per seed, floats >= 0 (each query scaled so its largest is 1, then round(w * 2^20)); unit by
        default; a query whose weights are all zero scores 0 everywhere.
        tolerance: a query whose largest change in a step is <= tolerance stops there, on its own; 0 runs max_iterations steps.
        -> float64 [B][n] scores (p / 2^40, exact), or with top_k (ids int64 [B][k], scores float64 [B][k], counts int32 [B]):
        the vertices of positive score by (score descending, vertex ascending), (-1, -inf) past the count.
        relation_types (a graph built with types only): None — the untyped run, today's code path — or the
        relation types each query may cross, as neighbourhood takes them: one iterable of type ids as one filter for every
        query, a sequence of B iterables, or a uint32 array [B] of masks.  Query q then runs the same rule on the graph of the
        edges whose mask shares a type with its filter, each at its full weight: its weighted degrees are those of that graph,
        and a vertex without an allowed edge keeps its mass.  A pair's mask is the OR and its weight the sum over its
        duplicates, so a pair that carries types {0, 1} is crossed at its whole weight under filter {0}: per-type weights are
        not kept.  Row q equals the untyped call on the filtered pair list, bit for bit; an empty filter leaves p = t.
        as_device=True leaves the results on the GPU.  ValueError for a negative or non-finite weight, a vertex outside [0, n),
        more than 64 seeds, relation_types on a graph without masks, a type outside [0, 32) or a filter count other than 1 or B."""
        a, tol = self._check_run(damping, max_iterations, tolerance, top_k, self.n)
        if relation_types is not None and not hasattr(seeds, "shape"):
            seeds = list(seeds)
        filters = self._typed_filters(relation_types, seeds)
        with self.torch.cuda.device(self.device):
            sd, wd = self._seed_tensors(seeds, seed_weights)
            return self._ranked(sd, wd, a, tol, max_iterations, None if top_k is None else int(top_k), as_device, filters=filters)

    def retrieve(self, index, queries, seeds_per_query: int = 5, top_k: int = 10, damping: float = 0.85, max_iterations: int = 20,
                 tolerance: float = 0.0, as_device: bool = False, relation_types=None):
        """Graph retrieval for embedded queries: row i of `index` (a FlatIndexF16) is the embedding of vertex i; each query's
        seeds are the index's own top-`seeds_per_query` (id, score) answer, the scores clipped at 0 as weights, taken on the
        device — the answer feeds rarc_ppr_seed directly, nothing leaves HBM between the search and the ranking.
        relation_types: as personalized_pagerank takes it, one filter for every query or one per query.
        -> (ids, scores, counts) as personalized_pagerank(top_k=top_k)."""
        self._check_index(index, seeds_per_query)
        a, tol = self._check_run(damping, max_iterations, tolerance, top_k, self.n)
        filters = self._typed_filters(relation_types)
        sd, wd = self._index_seeds(index, queries, seeds_per_query)
        with self.torch.cuda.device(self.device):
            return self._ranked(sd, wd, a, tol, max_iterations, int(top_k), as_device, filters=filters)

    def _check_index(self, index, seeds_per_query):
        if int(index.ntotal) != self.n:
            raise ValueError(f"the index holds {int(index.ntotal)} rows and the graph {self.n} vertices: row i must be vertex i")
        if not 1 <= int(seeds_per_query) <= MAX_SEEDS:
            raise ValueError(f"seeds_per_query must lie in [1, {MAX_SEEDS}]")

    def _index_seeds(self, index, queries, seeds_per_query):
        """the index's own top-`seeds_per_query` answer as seed tensors: (ids, quantised weights), both on the device"""
        t = self.torch
        ids, scores = index.search_device(queries, int(seeds_per_query))
        with t.cuda.device(self.device):
            ids = ids.to(self.device)
            w = scores.to(device=self.device, dtype=t.float64)
            w = t.where((ids >= 0) & (w > 0), w, t.zeros_like(w))          # clipped at 0; a slot past ntotal carries nothing
            mx = w.max(dim=1, keepdim=True).values
            wd = t.round(w / t.where(mx > 0, mx, t.ones_like(mx)) * float(MAX_SEED_WEIGHT)).to(t.int32).contiguous()
            return ids.contiguous(), wd

    # ---------------------------------------------------------------------------------------------------------------- passages
    def _check_chunks(self, mentions, damping, max_iterations, tolerance, top_k):
        from .passages import MentionMap

        if not isinstance(mentions, MentionMap):
            raise ValueError("mentions must be a MentionMap")
        if mentions.n_entities != self.n:
            raise ValueError(f"the mention map is over {mentions.n_entities} entities and the graph has {self.n} vertices: entity i must be "
                             f"vertex i")
        if mentions.device != self.device:
            raise ValueError(f"the mention map lives on {mentions.device} and the graph on {self.device}")
        a, tol = self._check_run(damping, max_iterations, tolerance, None, self.n)
        mentions.check_top_k(top_k)
        return a, tol

    def rank_chunks(self, mentions, seeds, seed_weights=None, damping: float = 0.85, max_iterations: int = 20, tolerance: float = 0.0,
                    top_k=None, as_device: bool = False, relation_types=None):
        """personalized_pagerank, ending in chunks: the state of every query is pushed through `mentions` (a MentionMap over
        this graph's vertices), S(c) = (sum over c's mentions (e, w) of w * p(e)) >> 12, without leaving the device.
        -> float64 [B][n_chunks] scores (S / 2^28, exact), or with top_k (ids int64 [B][k], scores float64 [B][k], counts
        int32 [B]): the chunks of positive score by (score descending, chunk ascending), (-1, -inf) past the count — a chunk
        without mentions is never returned.  Every other argument as personalized_pagerank, relation_types included: the
        projection reads the typed state as it reads the untyped one."""
        a, tol = self._check_chunks(mentions, damping, max_iterations, tolerance, top_k)
        if relation_types is not None and not hasattr(seeds, "shape"):
            seeds = list(seeds)
        filters = self._typed_filters(relation_types, seeds)
        with self.torch.cuda.device(self.device):
            sd, wd = self._seed_tensors(seeds, seed_weights)
            return self._ranked(sd, wd, a, tol, max_iterations, None if top_k is None else int(top_k), as_device, mentions=mentions,
                                filters=filters)

    def retrieve_chunks(self, index, queries, mentions, seeds_per_query: int = 5, top_k: int = 10, damping: float = 0.85,
                        max_iterations: int = 20, tolerance: float = 0.0, as_device: bool = False, relation_types=None):
        """retrieve, ending in chunks: the seeds are the index's own top-`seeds_per_query` answer, the ranking is rank_chunks'.
        relation_types: as personalized_pagerank takes it.
        -> (ids, scores, counts) as rank_chunks(top_k=top_k)."""
        self._check_index(index, seeds_per_query)
        a, tol = self._check_chunks(mentions, damping, max_iterations, tolerance, top_k)
        filters = self._typed_filters(relation_types)
        sd, wd = self._index_seeds(index, queries, seeds_per_query)
        with self.torch.cuda.device(self.device):
            return self._ranked(sd, wd, a, tol, max_iterations, int(top_k), as_device, mentions=mentions, filters=filters)

    # ---------------------------------------------------------------------------------------------------------------- traversal
    def neighbourhood(self, seeds, hops: int = 2, max_vertices=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
        """The vertices within `hops` edges of each query's seeds, and how far each is (graph_db/neighbourhood.py).
        seeds: as personalized_pagerank takes them (no weights: a seed has hop 0); a query may have none.  0 <= hops <= 8.
        -> uint8 [B][n]: hop_q(v), 255 for "not within hops"; or with max_vertices (1 .. 65536) the tuple (ids int64 [B][max],
        hops int32 [B][max], counts int32 [B], hop_counts int32 [B][hops + 1]): each neighbourhood by (hop ascending, vertex
        ascending), cut at max_vertices, (-1, -1) past the count; hop_counts[q][h] = the vertices at hop h exactly, never cut.
        early_stop=True reads one word after every step and stops stepping once no query reached a new vertex: the same answer.
        relation_types (a graph built with types only): None — the untyped traversal — or the relation types each
        query may cross: one iterable of type ids as one filter for every query, a sequence of B iterables, or a uint32 array
        [B] of masks.  An edge is crossed iff its mask shares a type with the filter; a seed has hop 0 whatever the filter.
        ValueError for a seed outside [0, n), more than 64 seeds, negative hops, relation_types on a graph without masks, a type
        outside [0, 32) or a filter count other than 1 or B; RarcUnsupported for hops > 8 or max_vertices > 65536."""
        from . import neighbourhood as K

        return K.neighbourhood(self, seeds, hops=hops, max_vertices=max_vertices, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def expand(self, index, queries, seeds_per_query: int = 5, hops: int = 2, max_vertices=None, as_device: bool = False,
               early_stop: bool = False, relation_types=None):
        """neighbourhood for embedded queries: each query's seeds are the index's own top-`seeds_per_query` ids (row i of `index`
        is the embedding of vertex i), taken on the device — nothing leaves HBM between the search and the traversal."""
        from . import neighbourhood as K

        return K.expand(self, index, queries, seeds_per_query=seeds_per_query, hops=hops, max_vertices=max_vertices, as_device=as_device,
                        early_stop=early_stop, relation_types=relation_types)

    def neighbourhood_chunks(self, mentions, seeds, hops: int = 2, decay=None, top_k=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
        """neighbourhood, ending in chunks: S(c) = sum over c's mentions (e, w) with hop(e) <= hops of w * decay[hop(e)].
        decay: hops + 1 integers in [0, 2^16]; by default 4096 >> (2 h), a mention one hop nearer counts four times as much.
        -> float64 [B][n_chunks] scores (S / 2^28, exact), or with top_k (ids, scores, counts) as rank_chunks returns them:
        (score descending, chunk ascending), a chunk of score 0 never returned."""
        from . import neighbourhood as K

        return K.neighbourhood_chunks(self, mentions, seeds, hops=hops, decay=decay, top_k=top_k, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def expand_chunks(self, index, queries, mentions, seeds_per_query: int = 5, hops: int = 2, decay=None, top_k: int = 10,
                      as_device: bool = False, early_stop: bool = False, relation_types=None):
        """expand, ending in chunks -> (ids, scores, counts) as neighbourhood_chunks(top_k=top_k)."""
        from . import neighbourhood as K

        return K.expand_chunks(self, index, queries, mentions, seeds_per_query=seeds_per_query, hops=hops, decay=decay, top_k=top_k,
                               as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def subgraph(self, seeds, hops: int = 2, max_vertices: int = 4096, max_edges: int = 16384, relations=None, as_device: bool = False,
                 early_stop: bool = False, relation_types=None):
        """The neighbourhood and the relations inside it, from one traversal.
        relations: a RelationList over this graph's vertices — the caller's table, rows (a, b) in any orientation, repeats and
        a == b allowed — or None for the graph's own normalised pair list.  A row's level is max(hop(a), hop(b)); it is listed
        iff that is <= hops.
        -> the named tuple (vertex_ids, vertex_hops, vertex_counts, hop_counts) as neighbourhood(max_vertices=...) returns them,
        then edge_ids int64 [B][max_edges] (row numbers of the relation list), edge_ends int64 [B][max_edges][2], edge_levels
        int32 [B][max_edges], edge_counts int32 [B], edge_level_counts int32 [B][hops + 1], and edge_weights [B][max_edges] when
        the list has weights (0 past the count): each list by (level ascending, row ascending), cut at max_edges (1 .. 65536),
        -1 past the count; edge_level_counts[q][h] = the rows at level h exactly, never cut.
        relation_types: as neighbourhood takes it; a row (a, b, t) is then listed for q only if q's filter holds t, so
        `relations` must carry types (None: the graph's own pairs, a pair listed iff its mask shares a type with the filter).
        ValueError for max_edges < 1, a relation list over other entities or on another device, or relation_types with a
        RelationList without types; RarcUnsupported for max_edges > 65536."""
        from . import neighbourhood as K

        return K.subgraph(self, seeds, hops=hops, max_vertices=max_vertices, max_edges=max_edges, relations=relations, as_device=as_device,
                          early_stop=early_stop, relation_types=relation_types)

    def neighbourhood_edges(self, seeds, hops: int = 2, max_edges: int = 16384, relations=None, as_device: bool = False,
                            early_stop: bool = False, relation_types=None):
        """The edge part of subgraph alone -> the named tuple (edge_ids, edge_ends, edge_levels, edge_counts, edge_level_counts,
        edge_weights or None)."""
        from . import neighbourhood as K

        return K.neighbourhood_edges(self, seeds, hops=hops, max_edges=max_edges, relations=relations, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def expand_subgraph(self, index, queries, seeds_per_query: int = 5, hops: int = 2, max_vertices: int = 4096, max_edges: int = 16384,
                        relations=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
        """subgraph for embedded queries: the seeds are the index's own top-`seeds_per_query` ids, as expand takes them."""
        from . import neighbourhood as K

        return K.expand_subgraph(self, index, queries, seeds_per_query=seeds_per_query, hops=hops, max_vertices=max_vertices, max_edges=max_edges,
                                 relations=relations, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def shortest_paths(self, sources, pairs, max_length: int = 4, max_vertices: int = 4096, max_edges: int = 16384, relations=None,
                       as_device: bool = False, early_stop: bool = False, relation_types=None):
        """How sources are connected: every shortest path of at most `max_length` edges between the two sources of each pair,
        MATCH p = allShortestPaths((a)-[*..L]-(b)), from one traversal of all sources.
        sources: 1 .. 256 seed sets as neighbourhood takes them (a set may be empty).  pairs: [np][2] indices into `sources`,
        1 <= np <= 256; ia == ib and repeats are allowed.  0 <= max_length <= 8.
        d = the fewest edges between any vertex of A and any of B, -1 if more than max_length; v is on the paths at position i
        iff hop_A(v) == i and hop_B(v) == d - i; a row of `relations` is at level i + 1 iff it joins positions i and i + 1.
        -> the named tuple (distances int32 [np], vertex_ids, vertex_positions, vertex_counts, position_counts) shaped as
        neighbourhood(max_vertices=...) shapes its lists, then the edge fields exactly as neighbourhood_edges returns them.
        relation_types: None or ONE filter (an iterable of type ids) for the whole call — every source traverses under it, so
        hop_A(v) + hop_B(v) == d stays valid — and a relation row additionally needs its type in the filter.
        ValueError for a seed outside [0, n), more than 64 seeds, a pair index outside [0, ns), a negative length or per-query
        filters; RarcUnsupported for max_length > 8, more than 256 sources or pairs, or a cap above 65536."""
        from . import neighbourhood as K

        return K.shortest_paths(self, sources, pairs, max_length=max_length, max_vertices=max_vertices, max_edges=max_edges,
                                relations=relations, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    def path_chunks(self, mentions, sources, pairs, max_length: int = 4, decay=None, top_k=None, as_device: bool = False,
                    early_stop: bool = False, relation_types=None):
        """shortest_paths, ending in chunks: S_p(c) = sum over c's mentions (e, w) with e on p's paths of w * decay[position(e)],
        decay of max_length + 1 entries -> scores float64 [np][n_chunks], or with top_k (ids, scores, counts), as
        neighbourhood_chunks shapes them."""
        from . import neighbourhood as K

        return K.path_chunks(self, mentions, sources, pairs, max_length=max_length, decay=decay, top_k=top_k, as_device=as_device,
                             early_stop=early_stop, relation_types=relation_types)

    def connect(self, index, queries, seeds_per_query: int = 5, max_length: int = 4, max_vertices: int = 4096, max_edges: int = 16384,
                relations=None, as_device: bool = False, early_stop: bool = False, relation_types=None):
        """shortest_paths between the entities a query links to: each query's seeds are the index's own top-`seeds_per_query`
        ids, as expand takes them; every seed is a one-vertex source and the pairs are all i < j within a query (2 <=
        seeds_per_query <= 23), cut into launches of at most 256 sources and pairs.
        -> the fields of shortest_paths, one row per pair, then pair_query int32 [np] (the query of a pair) and pair_ends int64
        [np][2] (its two seed vertices)."""
        from . import neighbourhood as K

        return K.connect(self, index, queries, seeds_per_query=seeds_per_query, max_length=max_length, max_vertices=max_vertices,
                         max_edges=max_edges, relations=relations, as_device=as_device, early_stop=early_stop, relation_types=relation_types)

    # ---------------------------------------------------------------------------------------------------------------- components
    def components(self, as_device: bool = False):
        """The connected components of the graph (graph_db/components.py) -> Components(labels int64 [n]: the
        smallest vertex of v's component; dense int32 [n]: that label's rank among the distinct labels; sizes int64
        [n_components] by dense id; n_components; largest = (label, size), among equals the smallest label; rounds).
        Computed on the first call and kept: the graph never changes.  as_device=True returns device tensors — the labels are
        what merge_plan takes."""
        from . import components as C

        return C.graph_components(self, as_device=as_device)

    def component_of(self, vertices):
        """The label of each vertex's component, from the kept labels: an int for one vertex, else an int64 array.  ValueError
        for a vertex outside [0, n)."""
        from . import components as C

        return C.component_of(self, vertices)

    def same_component(self, a, b):
        """Whether any path joins a and b (vertices, or arrays of them): PPR mass, k-hop levels and shortest paths never cross a
        component.  ValueError for a vertex outside [0, n)."""
        from . import components as C

        return C.same_component(self, a, b)


def personalized_pagerank(n: int, pairs, seeds, weights=None, device: int = 0, types=None, **kw):
    """The one-shot form: EntityGraph(n, pairs, weights, types, device).personalized_pagerank(seeds, **kw).  types: one relation
    type per pair, as k_hop takes it; relation_types= needs it, and is checked before the graph is built: a bad filter raises
    with no device visible."""
    from .neighbourhood import _check_one_shot_types

    if kw.get("relation_types") is not None and not hasattr(seeds, "shape"):
        seeds = list(seeds)
    _check_one_shot_types(types, kw, None if hasattr(seeds, "is_cuda") else len(seeds))
    return EntityGraph(n, pairs, weights=weights, types=types, device=device).personalized_pagerank(seeds, **kw)
