"""Graph ingest, on the MI355X (csrc/merge.hip, its last section): graphs and mention maps built from raw extraction rows on the
device, and extended by a batch without a rebuild from host arrays.

What it replaces in the reference: `store_graph(documents)` (event_graphrag_neo4j.py) is called per batch of documents and MERGEs
chunks, mentions, entities and relations into what is there (`_store_mentions`, `_store_entity_relations`,
`_create_chunk_entity_relations`).  The host constructors `EntityGraph(n, pairs, ...)` and `MentionMap(...)` normalise with
np.unique / bincount once and can never be added to; here the rows — in any orientation, with duplicates, typed and weighted — go
through one key kernel, rarc_sort_reduce's sort and segmented sum and a writer, and the lists `EntityGraph.from_device` and
`MentionMap.from_device_csr` adopt come out: `EntityGraph.from_rows`, `graph.extended`, `MentionMap.from_rows`,
`mentions.extended`, `relations.extended`.  An extension returns a NEW object; the receiver is not modified (the contract of
`merge_entities`), so searches in flight on the old one are unaffected.

The rule is in integers (restated by tests/ingest_ref.py): the results are the same bytes for any order of the rows
and from run to run.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import ctypes

import numpy as np

from ....hip import binding as B
from .communities import MAX_VERTICES
from .passages import MAX_CHUNKS, MAX_MENTION_WEIGHT

MAX_COUNT = 1 << 31            # base + new rows < 2^31 (rarc_sort_reduce's count limit)
MAX_EDGE_WEIGHT = 1 << 32      # a summed edge weight stays below this
MAX_TOTAL_WEIGHT = 1 << 31     # the total edge weight, as EntityGraph limits it
PAIR_KINDS = ("out_of_range", "self_loop", "zero_weight", "bad_type")
MENTION_KINDS = ("chunk_out_of_range", "entity_out_of_range", "bad_weight")


def limits() -> dict:
    """The constants of the ingest kernels (csrc/merge.hip): the relation types a mask holds, the bits of a mention weight, the
    split degree of a chunk and the limit on base + new rows."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_ingest_limits(out), "rarc_ingest_limits")
    return {"types": out[0], "mention_weight_bits": out[1], "split_degree": out[2], "max_count": 1 << out[3]}


def _is_device(x) -> bool:
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def check_on_invalid(on_invalid) -> None:
    if on_invalid not in ("raise", "skip"):
        raise ValueError(f"on_invalid must be 'raise' or 'skip', got {on_invalid!r}")


def check_rows(rows, what: str = "rows"):
    """-> (rows, r): host rows as a contiguous int64 [r][2] array, device rows as they are; ValueError for another shape or dtype.
    The VALUES are not looked at: the kernel counts what it skips."""
    if _is_device(rows):
        import torch

        if rows.ndim != 2 or rows.shape[1] != 2 or rows.dtype != torch.int64:
            raise ValueError(f"expected an int64 [r][2] tensor of {what}, got {rows.dtype} {tuple(rows.shape)}")
        return rows, int(rows.shape[0])
    arr = np.asarray(rows.cpu().numpy() if hasattr(rows, "cpu") else rows)
    if arr.size == 0:
        arr = np.zeros((0, 2), np.int64)
    if arr.ndim != 2 or arr.shape[1] != 2:
        raise ValueError(f"expected [r][2] {what}, got an array of shape {arr.shape}")
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{what} must be integers, got {arr.dtype}")
    return np.ascontiguousarray(arr.astype(np.int64)), int(arr.shape[0])


def check_values(x, r: int, what: str, signed: bool):
    """one integer per row -> host: an int32 [r] array (signed: a type, anything outside int32 becomes -1; else the uint32 bits of
    a weight in [0, 2^32)); a device tensor: as it is, int32 [r].  ValueError for another shape, a float that is no integer, or a
    weight outside [0, 2^32)"""
    if x is None:
        return None
    if _is_device(x):
        import torch

        if tuple(x.shape) != (r,) or x.dtype != torch.int32:
            raise ValueError(f"device {what} must be an int32 [{r}] tensor" + ("" if signed else " (the uint32 bits)") + f", got {x.dtype} {tuple(x.shape)}")
        return x
    a = np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    if a.shape != (r,):
        raise ValueError(f"expected {r} {what}, one per row, got an array of shape {a.shape}")
    if a.dtype == np.bool_ or (r and not np.all(a == np.floor(a))):
        raise ValueError(f"{what} must be integers")
    a = a.astype(np.int64)
    if signed:
        return np.ascontiguousarray(np.where((a < -(1 << 31)) | (a >= 1 << 31), -1, a).astype(np.int32))
    if r and (a.min() < 0 or a.max() >= MAX_EDGE_WEIGHT):
        raise ValueError(f"{what} must be integers in [0, 2^32)")
    return np.ascontiguousarray(a.astype(np.uint32).view(np.int32))


def _check_count(base: int, r: int, what: str) -> None:
    if base + r >= MAX_COUNT:
        raise B.RarcUnsupported(f"{base} resident and {r} new {what}: the kernels take base + new rows < 2^31")


def _require_device():
    import torch

    if not torch.cuda.is_available():
        raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
    return torch, B.load_library()


def _upload(torch, x, dev):
    if x is None:
        return None
    if isinstance(x, torch.Tensor):
        if x.device != dev:
            raise ValueError(f"an input lives on {x.device} and the result on {dev}")
        return x.contiguous()
    return torch.from_numpy(x).to(dev)


def _ptr(x):
    return None if x is None or x.numel() == 0 else x.data_ptr()


def _refuse_skipped(on_invalid, skipped: dict, what: str) -> None:
    bad = {k: v for k, v in skipped.items() if v}
    if bad and on_invalid == "raise":
        raise ValueError(f"{sum(bad.values())} {what} outside the rule: " + ", ".join(f"{k}={v}" for k, v in bad.items()) +
                         " (on_invalid='skip' leaves them out and reports the counts)")


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def check_pair_arguments(n, rows, weights, types, base=None, on_invalid="raise"):
    """Everything about a from_rows / extended call that needs no device -> (n, rows, r, weights, types).  ValueError for a bad
    on_invalid, shapes and dtypes, n below the receiver's, a typed receiver extended with untyped rows or the reverse;
    RarcUnsupported for n or base + r past the kernels' limits."""
    check_on_invalid(on_invalid)
    n = int(n)
    rows, r = check_rows(rows, "rows")
    weights = check_values(weights, r, "weights", signed=False)
    types = check_values(types, r, "types", signed=True)
    if n < 2:
        raise ValueError("a graph needs at least 2 vertices")
    if n >= MAX_VERTICES:
        raise B.RarcUnsupported(f"n={n}: the kernels take n < 2^31 - 1 vertices")
    if base is not None:
        if n < base.n:
            raise ValueError(f"n={n} is smaller than the graph's {base.n} vertices: an extension never drops a vertex")
        if base.typed != (types is not None):
            raise ValueError("the graph carries relation types and the rows do not" if base.typed else
                             "the rows carry relation types and the graph does not: a mask cannot be made up for the resident edges")
    _check_count(0 if base is None else base.m, r, "pairs")
    return n, rows, r, weights, types


def ingest_pairs(n, rows, weights=None, types=None, base=None, device: int = 0, on_invalid: str = "raise"):
    """rarc_ingest_pairs -> (pairs int64 [m][2], weights int32 [m] (uint32 bits) or None in unit mode, masks int32 [m] or None,
    skipped {kind: count}): device tensors as EntityGraph.from_device adopts them.  base: an EntityGraph to extend, or None."""
    n, rows, r, weights, types = check_pair_arguments(n, rows, weights, types, base, on_invalid)
    torch, lib = _require_device()
    dev = base.device if base is not None else next((x.device for x in (rows, weights, types) if _is_device(x)), torch.device("cuda", device))
    m0 = 0 if base is None else base.m
    if m0 + r < 1:
        raise ValueError("a graph needs at least 1 edge")
    with torch.cuda.device(dev):
        rows, weights, types = (_upload(torch, x, dev) for x in (rows, weights, types))
        bp, bw, bm = (None, None, None) if base is None else (base._pairs, base._pair_weights, base._type_masks)
        typed = types is not None or bm is not None
        unit = weights is None and bw is None
        cap = m0 + r
        ws = torch.empty(int(lib.rarc_ingest_pairs_workspace_bytes(m0, r)), dtype=torch.uint8, device=dev)
        pairs = torch.empty((cap, 2), dtype=torch.int64, device=dev)
        out_w = None if unit else torch.empty(cap, dtype=torch.int32, device=dev)
        out_m = torch.empty(cap, dtype=torch.int32, device=dev) if typed else None
        out8 = torch.empty(8, dtype=torch.int64, device=dev)
        B.check(lib.rarc_ingest_pairs(_ptr(rows), _ptr(weights), _ptr(types), r, _ptr(bp), _ptr(bw), _ptr(bm), m0, n, ws.data_ptr(), ws.numel(),
                                      pairs.data_ptr(), _ptr(out_w), _ptr(out_m), out8.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
                "rarc_ingest_pairs")
        counts = out8.tolist()
    edges, largest, total = counts[0], counts[1] & (2**64 - 1), counts[2]
    skipped = dict(zip(PAIR_KINDS, counts[3:7]))
    if counts[7]:
        raise B.RarcError(f"rarc_ingest_pairs skipped {counts[7]} resident pairs outside i < j < n, weight >= 1: the graph's pair list is damaged")
    _refuse_skipped(on_invalid, skipped, "rows")
    if edges < 1:
        raise ValueError("a graph needs at least 1 edge")
    if largest >= MAX_EDGE_WEIGHT:
        raise B.RarcUnsupported(f"the weights of an edge add up to {largest}: an edge weight must stay below 2^32")
    if total >= MAX_TOTAL_WEIGHT:
        raise B.RarcUnsupported("the total edge weight must stay below 2^31 (every weighted degree then fits 32 bits)")
    return pairs[:edges], None if out_w is None else out_w[:edges], None if out_m is None else out_m[:edges], skipped


def graph_from_rows(cls, n, rows, weights=None, types=None, device: int = 0, on_invalid: str = "raise", base=None):
    pairs, w, masks, skipped = ingest_pairs(n, rows, weights, types, base=base, device=device, on_invalid=on_invalid)
    graph = cls.from_device(int(n), pairs, w, masks)
    graph.skipped = skipped
    return graph


# ---- mentions ----------------------------------------------------------------------------------------------------------------------
def check_mention_arguments(n_chunks, n_entities, rows, weights, base=None, on_invalid="raise"):
    """Everything about a MentionMap.from_rows / extended call that needs no device -> (n_chunks, n_entities, rows, r, weights)."""
    check_on_invalid(on_invalid)
    n_chunks, n_entities = int(n_chunks), int(n_entities)
    rows, r = check_rows(rows, "(chunk, entity) mentions")
    weights = check_values(weights, r, "weights", signed=False)
    if n_chunks < 1:
        raise ValueError("a mention map needs at least 1 chunk")
    if n_chunks >= MAX_CHUNKS:
        raise B.RarcUnsupported(f"MentionMap(n_chunks={n_chunks}): the kernels take n_chunks < 2^31 - 1")
    if n_entities < 1:
        raise ValueError("a mention map needs at least 1 entity")
    if n_entities >= MAX_VERTICES:
        raise B.RarcUnsupported(f"MentionMap(n_entities={n_entities}): the kernels take n_entities < 2^31 - 1")
    if base is not None:
        if n_chunks < base.n_chunks:
            raise ValueError(f"n_chunks={n_chunks} is smaller than the map's {base.n_chunks} chunks: an extension never drops a chunk")
        if n_entities < base.n_entities:
            raise ValueError(f"n_entities={n_entities} is smaller than the map's {base.n_entities} entities: an extension never drops an entity")
    _check_count(0 if base is None else base.nnz, r, "mentions")
    return n_chunks, n_entities, rows, r, weights


def mentions_from_rows(cls, n_chunks, n_entities, rows, weights=None, device: int = 0, on_invalid: str = "raise", base=None):
    n_chunks, n_entities, rows, r, weights = check_mention_arguments(n_chunks, n_entities, rows, weights, base, on_invalid)
    torch, lib = _require_device()
    dev = base.device if base is not None else next((x.device for x in (rows, weights) if _is_device(x)), torch.device("cuda", device))
    nnz0 = 0 if base is None else base.nnz
    if nnz0 + r < 1:
        raise ValueError("a mention map needs at least 1 mention (nnz >= 1)")
    with torch.cuda.device(dev):
        rows, weights = _upload(torch, rows, dev), _upload(torch, weights, dev)
        cap = nnz0 + r
        ws = torch.empty(int(lib.rarc_ingest_mentions_workspace_bytes(n_chunks, nnz0, r)), dtype=torch.uint8, device=dev)
        row_ptr = torch.empty(n_chunks + 1, dtype=torch.int64, device=dev)
        ent, w = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        split = torch.empty(n_chunks, dtype=torch.int32, device=dev)
        out8 = torch.empty(8, dtype=torch.int64, device=dev)
        brp, be, bw, bc = (None, None, None, 0) if base is None else (base._row_ptr, base._ent, base._w, base.n_chunks)
        B.check(lib.rarc_ingest_mentions(_ptr(rows), _ptr(weights), r, _ptr(brp), _ptr(be), _ptr(bw), bc, nnz0, n_chunks, n_entities, ws.data_ptr(),
                                         ws.numel(), row_ptr.data_ptr(), ent.data_ptr(), w.data_ptr(), split.data_ptr(), out8.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream), "rarc_ingest_mentions")
        counts = out8.tolist()
    nnz, largest, n_split = counts[0], counts[1] & (2**64 - 1), counts[2]
    skipped = dict(zip(MENTION_KINDS, counts[3:6]))
    if counts[7]:
        raise B.RarcError(f"rarc_ingest_mentions skipped {counts[7]} resident mentions outside the rule: the mention map is damaged")
    _refuse_skipped(on_invalid, skipped, "mentions")
    if nnz < 1:
        raise ValueError("a mention map needs at least 1 mention (nnz >= 1)")
    if largest >= MAX_MENTION_WEIGHT:                                   # checked on the device's own maximum, before anything is returned
        raise B.RarcUnsupported(f"the weights of a (chunk, entity) add up to {largest}: the sum must stay below 2^12 = {MAX_MENTION_WEIGHT}")
    out = cls.from_device_csr(n_chunks, n_entities, row_ptr, ent[:nnz], w[:nnz], split[:n_split] if n_split else None)
    out.skipped = skipped
    return out


# ---- relations ---------------------------------------------------------------------------------------------------------------------
def relations_extended(relations, rows, weights=None, types=None, n_entities=None):
    """A new RelationList: the receiver's rows, then `rows` — existing rows keep their row numbers.  Concatenated on the device, no
    kernel.  ValueError when the rows carry weights or types and the receiver does not, or the reverse."""
    from .neighbourhood import MAX_RELATIONS, check_type_ids

    rows, r = check_rows(rows, "relations")
    n_entities = relations.n_entities if n_entities is None else int(n_entities)
    if n_entities < relations.n_entities:
        raise ValueError(f"n_entities={n_entities} is smaller than the list's {relations.n_entities} entities")
    if (weights is not None) != (relations._weights is not None):
        raise ValueError("the relation list carries weights and the rows do not" if weights is None else
                         "the rows carry weights and the relation list does not")
    if (types is not None) != relations.typed:
        raise ValueError("the relation list carries types and the rows do not" if types is None else "the rows carry types and the relation list does not")
    if relations.r + r >= MAX_RELATIONS:
        raise B.RarcUnsupported(f"RelationList of {relations.r + r} rows: the kernels take r < 2^31 - 1")
    if weights is not None:
        shape = tuple(weights.shape) if hasattr(weights, "shape") else np.asarray(weights).shape
        if tuple(shape) != (r,):
            raise ValueError(f"expected {r} numeric weights, got an array of shape {tuple(shape)}")
    if types is not None:
        types = check_type_ids(types.cpu().numpy() if hasattr(types, "cpu") else types, r, "row")
    torch, _ = _require_device()
    dev = relations.device
    with torch.cuda.device(dev):
        out = type(relations).__new__(type(relations))
        out.n_entities, out.r, out.device = n_entities, relations.r + r, dev
        out._pairs = torch.cat([relations._pairs, _upload(torch, rows, dev)])
        out._weights = out._types = None
        if weights is not None:
            w = weights if isinstance(weights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(weights)))
            out._weights = torch.cat([relations._weights, w.to(device=dev, dtype=relations._weights.dtype)])
        if types is not None:
            out._types = torch.cat([relations._types, torch.from_numpy(types).to(dev)])
    return out
