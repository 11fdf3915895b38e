"""Passage retrieval from the entity graph, on the MI355X (csrc/ppr.hip, its last section): the PageRank mass of the entities
pushed through the mention links onto the chunks, and the chunks ranked.

What it replaces: the reference stores `(chunk)-[:MENTIONS]->(entity)` (event_graphrag_neo4j.py:508-536), and every PPR-based
graph retriever (HippoRAG's, upstream RAG-ARC's) ends by summing, per passage, the PageRank of the entities it mentions.  With
`EntityGraph.personalized_pagerank(top_k=None)` that is a [B][n] float64 matrix pulled to the host, a sparse product and a sort;
here `MentionMap` keeps the links resident as a CSR by chunk and `EntityGraph.rank_chunks` / `.retrieve_chunks` project and rank
next to the PPR state, without leaving HBM.

The rule is fixed point (restated by tests/passage_ref.py): S(c) = (sum over c's mentions (e, w) of w * p(e)) >> 12
with integer weights w in [1, 2^12), the score S / 2^28 — the same bits for any order of the mentions and any batch.  Only the sum
is offered: a length normalisation is the caller's, through w.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import ctypes

import numpy as np

from ....hip import binding as B

MAX_MENTION_WEIGHT = 1 << 12   # a (chunk, entity) weight, duplicates summed, stays below this
SCORE_SHIFT = 28               # score = S / 2^28
MAX_CHUNKS = (1 << 31) - 1     # n_chunks < 2^31 - 1: a chunk id is an int32 on the device
MAX_TOPK_CHUNKS = 1 << 24      # the top-k key carries the chunk in 24 bits
MAX_TOP_K = 8192


def limits() -> dict:
    """The constants of the projection (csrc/ppr.hip): the most mentions a single wave walks (a chunk of more is split across a
    workgroup), the bits of a mention weight, the shift of a score and the bits of a chunk in the top-k key."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_ppr_chunks_limits(out), "rarc_ppr_chunks_limits")
    return {"split_degree": out[0], "weight_bits": out[1], "score_shift": out[2], "topk_chunk_bits": out[3]}


def mention_csr(n_chunks: int, n_entities: int, mentions, weights=None, split_degree: int = 64):
    """Host mentions -> (row_ptr int64 [n_chunks + 1], entities int32 [nnz], weights uint32 [nnz], split int32 [...]): the
    duplicates of a (chunk, entity) merged (their weights add up), sorted by (chunk, entity); `split` lists the chunks of more
    than `split_degree` mentions.  ValueError / RarcUnsupported, naming the limit, for an id out of range, a weight that is no
    integer >= 1, a summed weight >= 2^12, or no mention at all."""
    n_chunks, n_entities = int(n_chunks), int(n_entities)
    if n_chunks < 1:
        raise ValueError("a mention map needs at least 1 chunk")
    if n_chunks >= MAX_CHUNKS:
        raise B.RarcUnsupported(f"MentionMap(n_chunks={n_chunks}): the kernels take n_chunks < 2^31 - 1")
    if n_entities < 1:
        raise ValueError("a mention map needs at least 1 entity")
    arr = np.asarray(mentions)
    if arr.size == 0:
        arr = np.zeros((0, 2), np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError(f"expected [nnz][2] (chunk, entity) mentions, got an array of shape {arr.shape}")
    if not np.issubdtype(arr.dtype, np.integer) and not np.all(arr == np.floor(arr)):
        raise ValueError("mentions must be integers")
    arr = arr.astype(np.int64)
    if arr.shape[0] < 1:
        raise ValueError("a mention map needs at least 1 mention (nnz >= 1)")
    if weights is None:
        w = np.ones(arr.shape[0], np.int64)
    else:
        w = np.asarray(weights)
        if w.shape != (arr.shape[0],):
            raise ValueError(f"expected {arr.shape[0]} weights, got an array of shape {w.shape}")
        if not np.all(w == np.floor(w)) or w.min() < 1:
            raise ValueError("mention weights must be integers >= 1")
        if w.max() >= MAX_MENTION_WEIGHT:
            raise B.RarcUnsupported(f"a mention weight of {int(w.max())}: the weight of a (chunk, entity) must stay below 2^12 = {MAX_MENTION_WEIGHT}")
        w = w.astype(np.int64)
    if arr[:, 0].min() < 0 or arr[:, 0].max() >= n_chunks:
        raise ValueError(f"a mention names a chunk outside [0, {n_chunks})")
    if arr[:, 1].min() < 0 or arr[:, 1].max() >= n_entities:
        raise ValueError(f"a mention names an entity outside [0, {n_entities})")
    key, inverse = np.unique(arr[:, 0] * n_entities + arr[:, 1], return_inverse=True)      # sorted by (chunk, entity)
    wsum = np.bincount(inverse.ravel(), weights=w.astype(np.float64), minlength=key.shape[0]).astype(np.int64)
    if wsum.max() >= MAX_MENTION_WEIGHT:
        raise B.RarcUnsupported(f"the weights of a repeated (chunk, entity) add up to {int(wsum.max())}: the sum must stay below 2^12 = "
                                f"{MAX_MENTION_WEIGHT}")
    chunk = key // n_entities
    degree = np.bincount(chunk, minlength=n_chunks)
    row_ptr = np.zeros(n_chunks + 1, np.int64)
    np.cumsum(degree, out=row_ptr[1:])
    split = np.flatnonzero(degree > int(split_degree)).astype(np.int32)
    return row_ptr, (key % n_entities).astype(np.int32), wsum.astype(np.uint32), split


class MentionMap:
    """The links (chunk)-[:MENTIONS]->(entity), resident on the device as a CSR by chunk.
    mentions: an [nnz][2] array-like of (chunk, entity); weights: integers >= 1 per mention (unit by default) — how often the
    chunk mentions the entity, or any weight the caller prefers.  A repeated (chunk, entity) is one mention whose weights add
    up; every weight, summed, stays below 2^12."""

    def __init__(self, n_chunks: int, n_entities: int, mentions, weights=None, device: int = 0):
        import torch

        lim = limits()
        row_ptr, ent, w, split = mention_csr(n_chunks, n_entities, mentions, weights, split_degree=lim["split_degree"])
        if not torch.cuda.is_available():
            raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
        self.torch, self.lib = torch, B.load_library()
        self.n_chunks, self.n_entities, self.nnz = int(n_chunks), int(n_entities), int(ent.shape[0])
        self.split_degree = lim["split_degree"]
        self.device = torch.device("cuda", device)
        with torch.cuda.device(self.device):
            self._row_ptr = torch.from_numpy(row_ptr).to(self.device)
            self._ent = torch.from_numpy(ent).to(self.device)
            self._w = torch.from_numpy(w.view(np.int32)).to(self.device)
            self._split = torch.from_numpy(split).to(self.device) if split.size else None
        self.n_split = int(split.size)
        self._cws = None

    @classmethod
    def from_device_csr(cls, n_chunks: int, n_entities: int, row_ptr, entities, weights, split=None):
        """Adopts a CSR that is on a device already, in the form `mention_csr` produces (graph_db/merge.py builds a merged map
        this way): row_ptr int64 [n_chunks + 1], entities int32 [nnz] (each row ascending, no repeats), weights int32 [nnz]
        holding uint32 bits in [1, 2^12), split int32: the chunks of more than `split_degree` mentions, or None for none.  The
        producer answers for the contents; the kernels guard every index they read either way."""
        import torch

        n_chunks, n_entities = int(n_chunks), int(n_entities)
        if n_chunks < 1:
            raise ValueError("a mention map needs at least 1 chunk")
        if n_chunks >= MAX_CHUNKS:
            raise B.RarcUnsupported(f"MentionMap(n_chunks={n_chunks}): the kernels take n_chunks < 2^31 - 1")
        if n_entities < 1:
            raise ValueError("a mention map needs at least 1 entity")
        nnz = int(entities.shape[0]) if isinstance(entities, torch.Tensor) and entities.ndim == 1 else None
        want = ((row_ptr, torch.int64, n_chunks + 1), (entities, torch.int32, nnz), (weights, torch.int32, nnz))
        for x, dtype, length in want + (((split, torch.int32, None),) if split is not None else ()):
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.device == row_ptr.device and x.ndim == 1 and x.dtype == dtype
                    and (length is None or int(x.shape[0]) == length)):
                raise ValueError("expected device tensors on one device: row_ptr int64 [n_chunks + 1], entities int32 [nnz], weights "
                                 "int32 [nnz], split int32")
        if int(entities.shape[0]) < 1:
            raise ValueError("a mention map needs at least 1 mention (nnz >= 1)")
        self = cls.__new__(cls)
        self.torch, self.lib = torch, B.load_library()
        self.n_chunks, self.n_entities, self.nnz = n_chunks, n_entities, int(entities.shape[0])
        self.split_degree = limits()["split_degree"]
        self.device = row_ptr.device
        self._row_ptr, self._ent, self._w = row_ptr.contiguous(), entities.contiguous(), weights.contiguous()
        self.n_split = 0 if split is None else int(split.shape[0])
        self._split = split.contiguous() if self.n_split else None
        self._cws = None
        return self

    @classmethod
    def from_rows(cls, n_chunks: int, n_entities: int, rows, weights=None, device: int = 0, on_invalid: str = "raise"):
        """The map of raw (chunk, entity) rows, built on the device (graph_db/ingest.py): `rows` a host array-like
        or an int64 device tensor [r][2], `weights` integers per row (host, or a device int32 tensor of uint32 bits), 1 by
        default.  Equal to MentionMap(n_chunks, n_entities, rows, weights) where that takes the rows.  A row with a chunk outside
        [0, n_chunks), an entity outside [0, n_entities) or a weight outside [1, 2^12) is no mention: on_invalid="raise" raises
        ValueError naming the kinds and counts, "skip" leaves such rows out and reports {kind: count} as `.skipped`.
        ValueError for no mention at all, RarcUnsupported for a summed weight >= 2^12."""
        from . import ingest

        return ingest.mentions_from_rows(cls, n_chunks, n_entities, rows, weights=weights, device=device, on_invalid=on_invalid)

    def extended(self, rows, weights=None, n_chunks=None, n_entities=None, on_invalid: str = "raise"):
        """A NEW MentionMap over n_chunks >= self.n_chunks chunks and n_entities >= self.n_entities entities (default: as many):
        this map's mentions and `rows`, as from_rows takes them, folded together on the device.  This map is not modified."""
        from . import ingest

        return ingest.mentions_from_rows(type(self), self.n_chunks if n_chunks is None else n_chunks,
                                         self.n_entities if n_entities is None else n_entities, rows, weights=weights, on_invalid=on_invalid,
                                         base=self)

    def cooccurrence_pairs(self, weight: str = "count", min_weight: int = 1, max_mentions: int = 64, as_device: bool = False):
        """The edges of the co-occurrence projection (graph_db/cooccurrence.py): two entities are joined when a chunk
        mentions both, W(a, b) = the chunks that do (weight="count") or the sum of w_a * w_b over them (weight="product"); a chunk
        of more than max_mentions mentions gives nothing.  -> Cooccurrence(pairs int64 [m][2] by (a, b) with a < b, weights uint32
        [m], total_pairs, chunks_skipped, largest_weight); no edge is an empty answer."""
        from . import cooccurrence as C

        return C.cooccurrence_pairs(self, weight=weight, min_weight=min_weight, max_mentions=max_mentions, as_device=as_device)

    def cooccurrence(self, weight: str = "count", min_weight: int = 1, max_mentions: int = 64):
        """The co-occurrence projection as an EntityGraph over this map's entities, built on the device from cooccurrence_pairs.
        ValueError("no two entities share a chunk") when there is no edge."""
        from . import cooccurrence as C

        return C.cooccurrence(self, weight=weight, min_weight=min_weight, max_mentions=max_mentions)

    def check_top_k(self, top_k) -> None:
        if top_k is None:
            return
        if not 1 <= int(top_k) <= MAX_TOP_K:
            raise ValueError(f"top_k must lie in [1, {MAX_TOP_K}]")
        if self.n_chunks >= MAX_TOPK_CHUNKS:
            raise B.RarcUnsupported(f"top_k over n_chunks={self.n_chunks}: the top-k key carries the chunk in 24 bits, n_chunks < 2^24 = "
                                    f"{MAX_TOPK_CHUNKS}; ask for the scores (top_k=None) instead")

    def workspace(self, nq: int):
        """-> (pointer, bytes) of the chunk workspace for a launch batch of nq queries: whoever writes the chunk state S (rarc_ppr_chunks,
        rarc_khop_chunks) writes it there, and `ranked` reads it"""
        t, lib, nc = self.torch, self.lib, self.n_chunks
        need = int(lib.rarc_ppr_chunks_workspace_bytes(nc, nq))
        if need == 0:
            raise B.RarcError(f"rank_chunks: n_chunks={nc}, {nq} queries refused by rarc_ppr_chunks_workspace_bytes")
        if self._cws is None or self._cws.numel() < need:
            self._cws = None
            self._cws = t.empty(need, dtype=t.uint8, device=self.device)
        return self._cws.data_ptr(), self._cws.numel()

    def split_list(self):
        """-> (pointer or None, length) of the list of chunks of more than `split_degree` mentions"""
        return (self._split.data_ptr() if self._split is not None else None), self.n_split

    def project(self, n: int, m: int, nq: int, cur: int, ws, top_k):
        """The tail of one launch batch: the PPR state in `ws` (a device uint8 tensor, rarc_ppr_workspace_bytes) -> device tensors,
        scores float64 [nq][n_chunks] or (ids, scores, counts)"""
        t, lib, nc = self.torch, self.lib, self.n_chunks
        cws, cb = self.workspace(nq)
        stream = t.cuda.current_stream(self.device).cuda_stream
        split, n_split = self.split_list()
        B.check(lib.rarc_ppr_chunks(n, m, nq, cur, ws.data_ptr(), ws.numel(), self._row_ptr.data_ptr(), self._ent.data_ptr(), self._w.data_ptr(),
                                    nc, self.nnz, split, n_split, cws, cb, stream),
                "rarc_ppr_chunks")
        return self.ranked(nq, top_k)

    def ranked(self, nq: int, top_k):
        """The chunk state S of the workspace -> device tensors: scores float64 [nq][n_chunks] (S / 2^28), or (ids, scores, counts)"""
        t, lib, nc = self.torch, self.lib, self.n_chunks
        cws, cb = self.workspace(nq)
        stream = t.cuda.current_stream(self.device).cuda_stream
        if top_k is None:
            out = t.empty((nq, nc), dtype=t.float64, device=self.device)
            B.check(lib.rarc_ppr_chunks_scores(nc, nq, cws, cb, out.data_ptr(), stream), "rarc_ppr_chunks_scores")
            return out
        ids = t.empty((nq, top_k), dtype=t.int64, device=self.device)
        sc = t.empty((nq, top_k), dtype=t.float64, device=self.device)
        cnt = t.empty(nq, dtype=t.int32, device=self.device)
        B.check(lib.rarc_ppr_chunks_topk(nc, nq, top_k, cws, cb, ids.data_ptr(), sc.data_ptr(), cnt.data_ptr(), stream), "rarc_ppr_chunks_topk")
        return ids, sc, cnt
