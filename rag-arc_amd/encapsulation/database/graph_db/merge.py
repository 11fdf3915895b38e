"""Entity merging, on the MI355X (csrc/merge.hip): step 4 of the reference's entity de-duplication
(encapsulation/database/graph_db/Base_Neo4j.py:386-434).

What it replaces in the reference: `_merge_clusters` (:714-890) picks the richest member of every cluster as the primary,
re-creates every relationship of the others on it with apoc.create.relationship and DETACH DELETEs the others.  Steps 1-3
(`similar_pairs`, `entity_clusters`) end in labels; the graph step 4 leaves behind is what `EntityGraph`, `MentionMap` and
`RelationList` are queried as.  Here the step runs between them without leaving HBM: `merge_plan(labels)` picks the primaries and
numbers the survivors, `merge_entities(plan, graph, mentions, relations)` contracts the pair list, the mention CSR and the
relation table onto them and hands back new resident objects, and `deduplicate_entities(embeddings, ...)` runs steps 1-4 in one
call.

The rule is in integers (restated by tests/merge_ref.py): the results are the same bits for any order of the pairs
and mentions, and from run to run.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from ....hip import binding as B
from .communities import MAX_VERTICES
from .passages import MAX_MENTION_WEIGHT

MAX_KEY_BITS = 62              # rarc_sort_reduce: the bits of a key
MAX_COUNT = 1 << 31            # rarc_sort_reduce: count < 2^31
MAX_RICHNESS = 1 << 32         # a richness is an integer in [0, 2^32)

MergedEntities = collections.namedtuple("MergedEntities", ("plan", "graph", "mentions", "relations", "relation_rows", "dropped"))


def limits() -> dict:
    """The constants of rarc_sort_reduce (csrc/merge.hip): the keys of a tile, the bits a pass sorts by, the largest key_bits and
    the count limit."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_sort_reduce_limits(out), "rarc_sort_reduce_limits")
    return {"tile": out[0], "radix_bits": out[1], "max_key_bits": out[2], "max_count": 1 << out[3]}


def _require_device():
    import torch

    if not torch.cuda.is_available():
        raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
    return torch, B.load_library()


def sort_reduce(keys, values=None, key_bits: int = MAX_KEY_BITS, device: int = 0, as_device: bool = False):
    """np.unique + bincount on the device: the distinct keys ascending, the sum of the values of each, and the largest sum.
    keys: integers in [0, 2^key_bits), a host array or a device tensor (int64 or uint64 bits); values: integers in [0, 2^32) or
    None for 1 each.  -> (keys uint64 [u], sums uint64 [u], largest sum); device tensors hold the uint64 bits as int64."""
    key_bits = int(key_bits)
    if not 1 <= key_bits <= MAX_KEY_BITS:
        raise ValueError(f"key_bits must lie in [1, {MAX_KEY_BITS}]")
    on_device = hasattr(keys, "is_cuda") and keys.is_cuda
    if not on_device:
        keys = np.ascontiguousarray(np.asarray(keys).astype(np.uint64).view(np.int64))
        if keys.ndim != 1 or (keys.size and (keys.min() < 0 or int(keys.max()) >> key_bits)):
            raise ValueError(f"keys must be a vector of integers in [0, 2^{key_bits})")
    count = int(keys.shape[0])
    if not 1 <= count < MAX_COUNT:
        raise ValueError(f"{count} keys: 1 <= count < 2^31 are taken")
    if values is not None and not (hasattr(values, "is_cuda") and values.is_cuda):
        values = np.asarray(values)
        if values.shape != (count,) or not np.all(values == np.floor(values)) or values.min() < 0 or values.max() >= MAX_RICHNESS:
            raise ValueError(f"values must be {count} integers in [0, 2^32)")
        values = np.ascontiguousarray(values.astype(np.uint32).view(np.int32))
    torch, lib = _require_device()
    dev = keys.device if on_device else torch.device("cuda", device)
    with torch.cuda.device(dev):
        k = keys.contiguous() if on_device else torch.from_numpy(keys).to(dev)
        v = None if values is None else (values if isinstance(values, torch.Tensor) else torch.from_numpy(values)).to(dev).contiguous()
        if k.dtype != torch.int64 or (v is not None and (v.dtype != torch.int32 or tuple(v.shape) != (count,))):
            raise ValueError("device keys must be int64 [count] and device values int32 [count] (the unsigned bits)")
        ws = torch.empty(int(lib.rarc_sort_reduce_workspace_bytes(count)), dtype=torch.uint8, device=dev)
        ok, os_ = torch.empty(count, dtype=torch.int64, device=dev), torch.empty(count, dtype=torch.int64, device=dev)
        out2 = torch.empty(2, dtype=torch.int64, device=dev)
        B.check(lib.rarc_sort_reduce(k.data_ptr(), v.data_ptr() if v is not None else None, count, key_bits, ws.data_ptr(), ws.numel(),
                                     ok.data_ptr(), os_.data_ptr(), out2.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rarc_sort_reduce")
        distinct, largest = out2.tolist()
        ok, os_ = ok[:distinct], os_[:distinct]
        if as_device:
            return ok, os_, largest & (2**64 - 1)
        return ok.cpu().numpy().view(np.uint64), os_.cpu().numpy().view(np.uint64), largest & (2**64 - 1)


class MergePlan:
    """Which entity every entity becomes.  n: entities before, n_merged: after; primary [n]: old -> the old index of its primary;
    new_id [n]: old -> new; kept [n_merged]: new -> old, ascending (the rows of an embedding index compact with this list);
    removed [n - n_merged]: the others, ascending.  int64 numpy arrays, or device tensors when made with as_device=True; the
    map itself stays on the device for `merge_entities`."""

    def __init__(self, n, n_merged, primary, new_id, kept, removed, device, new_id_device):
        self.n, self.n_merged = int(n), int(n_merged)
        self.primary, self.new_id, self.kept, self.removed = primary, new_id, kept, removed
        self.device, self._new_id = device, new_id_device


def _check_labels(labels, richness):
    """-> (n, labels, richness) with host inputs as contiguous int64 / uint32-bits arrays; ValueError for what is no labelling"""
    def is_dev(x):
        return hasattr(x, "is_cuda") and x.is_cuda

    if is_dev(labels):
        import torch

        if labels.ndim != 1 or labels.dtype != torch.int64:
            raise ValueError(f"expected an int64 [n] tensor of labels, got {labels.dtype} {tuple(labels.shape)}")
    else:
        labels = np.asarray(labels.cpu().numpy() if hasattr(labels, "cpu") else labels)
        if labels.ndim != 1:
            raise ValueError(f"expected [n] labels, got an array of shape {labels.shape}")
        if labels.size and not np.issubdtype(labels.dtype, np.integer) and not np.all(labels == np.floor(labels)):
            raise ValueError("labels must be integers")
        labels = np.ascontiguousarray(labels.astype(np.int64))
    n = int(labels.shape[0])
    if n < 1:
        raise ValueError("a labelling needs at least 1 entity")
    if n >= MAX_VERTICES:
        raise B.RarcUnsupported(f"merge_plan(n={n}): the kernels take n < 2^31 - 1 entities")
    if not is_dev(labels) and (labels.min() < 0 or labels.max() >= n):
        raise ValueError(f"a label lies outside [0, {n})")
    if richness is not None:
        if is_dev(richness):
            if tuple(richness.shape) != (n,) or richness.dtype.is_floating_point:
                raise ValueError(f"expected {n} integer richness values, got {richness.dtype} {tuple(richness.shape)}")
        else:
            richness = np.asarray(richness.cpu().numpy() if hasattr(richness, "cpu") else richness)
            if richness.shape != (n,) or not np.all(richness == np.floor(richness)) or richness.min() < 0 or richness.max() >= MAX_RICHNESS:
                raise ValueError(f"richness must be {n} integers in [0, 2^32)")
            richness = np.ascontiguousarray(richness.astype(np.uint32).view(np.int32))
    return n, labels, richness


def merge_plan(labels, richness=None, device: int = 0, as_device: bool = False) -> MergePlan:
    """The primaries of a labelling and the numbering of the survivors.
    labels: int64 [n] with values in [0, n) — Louvain's, or any other classes — a host array or a device tensor, used where it
    is.  richness: integers in [0, 2^32) per entity (the reference counts descriptions + mentions + sources), all 0 by default.
    The primary of a class is its member of largest richness, among equals the smallest index; the primaries are numbered in
    ascending old index, so survivors keep their relative order.  ValueError for a label outside [0, n) or a richness that is
    no integer in [0, 2^32)."""
    n, labels, richness = _check_labels(labels, richness)
    torch, lib = _require_device()
    dev = labels.device if isinstance(labels, torch.Tensor) else torch.device("cuda", device)
    with torch.cuda.device(dev):
        if isinstance(labels, torch.Tensor):
            lab = labels.contiguous()
            if not bool(((lab >= 0) & (lab < n)).all().item()):
                raise ValueError(f"a label lies outside [0, {n})")
        else:
            lab = torch.from_numpy(labels).to(dev)
        rich = None
        if richness is not None:
            if isinstance(richness, torch.Tensor):
                r64 = richness.to(device=dev, dtype=torch.int64)
                if not bool(((r64 >= 0) & (r64 < MAX_RICHNESS)).all().item()):
                    raise ValueError(f"richness must be {n} integers in [0, 2^32)")
                rich = torch.where(r64 >= 1 << 31, r64 - MAX_RICHNESS, r64).to(torch.int32).contiguous()      # (the uint32 bits)
            else:
                rich = torch.from_numpy(richness).to(dev)
        ws = torch.empty(int(lib.rarc_merge_plan_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        primary, new_id, kept, removed = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4))
        count = torch.empty(1, dtype=torch.int64, device=dev)
        B.check(lib.rarc_merge_plan(lab.data_ptr(), rich.data_ptr() if rich is not None else None, n, ws.data_ptr(), ws.numel(), primary.data_ptr(),
                                    new_id.data_ptr(), kept.data_ptr(), removed.data_ptr(), count.data_ptr(),
                                    torch.cuda.current_stream(dev).cuda_stream), "rarc_merge_plan")
        n_c = int(count.item())
        kept, removed = kept[:n_c], removed[:n - n_c]
        out = (primary, new_id, kept, removed) if as_device else tuple(x.cpu().numpy() for x in (primary, new_id, kept, removed))
        return MergePlan(n, n_c, *out, device=dev, new_id_device=new_id)


def _check_inputs(plan, graph, mentions, relations):
    """ValueError for an input of another type, over another number of entities than the plan's, or on another device"""
    from .neighbourhood import RelationList
    from .pagerank import EntityGraph
    from .passages import MentionMap

    for what, x, kind, n in (("graph", graph, EntityGraph, getattr(graph, "n", None)),
                             ("mention map", mentions, MentionMap, getattr(mentions, "n_entities", None)),
                             ("relation list", relations, RelationList, getattr(relations, "n_entities", None))):
        if x is None:
            continue
        if not isinstance(x, kind):
            raise ValueError(f"the {what} must be a {kind.__name__}")
        if n != plan.n:
            raise ValueError(f"the {what} is over {n} entities and the plan over {plan.n}: entity i must be label i")
        if x.device != plan.device:
            raise ValueError(f"the {what} lives on {x.device} and the plan on {plan.device}")


def _input_device(*xs):
    for x in xs:
        index = getattr(getattr(x, "device", None), "index", None)          # (a numpy array's device is the string "cpu")
        if isinstance(index, int):
            return index
    return 0


def _merge_graph(lib, torch, plan, graph, dropped):
    dev, m = plan.device, graph.m
    ws = torch.empty(int(lib.rarc_merge_pairs_workspace_bytes(m)), dtype=torch.uint8, device=dev)
    pairs = torch.empty((m, 2), dtype=torch.int64, device=dev)
    weights = torch.empty(m, dtype=torch.int32, device=dev)
    out5 = torch.empty(5, dtype=torch.int64, device=dev)
    w = graph._pair_weights
    B.check(lib.rarc_merge_pairs(graph._pairs.data_ptr(), w.data_ptr() if w is not None else None, m, plan._new_id.data_ptr(), plan.n, ws.data_ptr(),
                                 ws.numel(), pairs.data_ptr(), weights.data_ptr(), out5.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
            "rarc_merge_pairs")
    m_c, largest, dropped["edges"], dropped["edge_weight"], bad = out5.tolist()
    if bad:
        raise B.RarcError(f"rarc_merge_pairs skipped {bad} pairs with an end outside [0, {plan.n}): the graph's pair list is damaged")
    if plan.n_merged < 2 or m_c < 1:
        return None                                                  # EntityGraph refuses such a graph
    if largest >= 1 << 32:
        raise B.RarcUnsupported(f"the weights of a merged edge add up to {largest}: an edge weight must stay below 2^32")
    from .pagerank import EntityGraph

    return EntityGraph.from_device(plan.n_merged, pairs[:m_c], weights[:m_c])


def _merge_mentions(lib, torch, plan, mentions):
    dev, nc, nnz = plan.device, mentions.n_chunks, mentions.nnz
    ws = torch.empty(int(lib.rarc_merge_mentions_workspace_bytes(nc, nnz)), dtype=torch.uint8, device=dev)
    row_ptr = torch.empty(nc + 1, dtype=torch.int64, device=dev)
    ent, w = torch.empty(nnz, dtype=torch.int32, device=dev), torch.empty(nnz, dtype=torch.int32, device=dev)
    split = torch.empty(nc, dtype=torch.int32, device=dev)
    out6 = torch.empty(6, dtype=torch.int64, device=dev)
    B.check(lib.rarc_merge_mentions(mentions._row_ptr.data_ptr(), mentions._ent.data_ptr(), mentions._w.data_ptr(), nc, nnz, plan._new_id.data_ptr(),
                                    plan.n, ws.data_ptr(), ws.numel(), row_ptr.data_ptr(), ent.data_ptr(), w.data_ptr(), split.data_ptr(),
                                    out6.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rarc_merge_mentions")
    nnz_c, largest, _, _, bad, n_split = out6.tolist()
    if bad:
        raise B.RarcError(f"rarc_merge_mentions skipped {bad} mentions outside the rule: the mention map is damaged")
    if largest >= MAX_MENTION_WEIGHT:                                   # checked on the device's own maximum, before anything is returned
        raise B.RarcUnsupported(f"the weights of a merged (chunk, entity) add up to {largest}: the sum must stay below 2^12 = {MAX_MENTION_WEIGHT}")
    from .passages import MentionMap

    return MentionMap.from_device_csr(nc, plan.n_merged, row_ptr, ent[:nnz_c], w[:nnz_c], split[:n_split] if n_split else None)


def _merge_relations(lib, torch, plan, relations, dropped):
    dev, r = plan.device, relations.r
    ws = torch.empty(int(lib.rarc_merge_relations_workspace_bytes(r)), dtype=torch.uint8, device=dev)
    table = torch.empty((r, 2), dtype=torch.int64, device=dev)
    rows = torch.empty(r, dtype=torch.int64, device=dev)
    out3 = torch.empty(3, dtype=torch.int64, device=dev)
    B.check(lib.rarc_merge_relations(relations._pairs.data_ptr(), r, plan._new_id.data_ptr(), plan.n, ws.data_ptr(), ws.numel(), table.data_ptr(),
                                     rows.data_ptr(), out3.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rarc_merge_relations")
    r_c, dropped["relations_internal"], dropped["relations_out_of_range"] = out3.tolist()
    rows = rows[:r_c]
    if r_c < 1:
        return None, rows                                            # RelationList refuses an empty table
    from .neighbourhood import RelationList

    weights = None if relations._weights is None else relations._weights[rows]
    return RelationList(plan.n_merged, table[:r_c], weights=weights, device=dev.index), rows


def merge_entities(plan_or_labels, graph=None, mentions=None, relations=None, richness=None, as_device: bool = False) -> MergedEntities:
    """Contracts a graph, a mention map and a relation list (each optional, none modified) onto the survivors of a plan.
    plan_or_labels: a MergePlan, or labels (with `richness`) as merge_plan takes them.
    -> MergedEntities(plan, graph, mentions, relations, relation_rows, dropped):
    graph: a new EntityGraph over n_merged vertices — both ends mapped, a pair inside one entity dropped, equal pairs merged with
      added weights, the pair list by (i, j) — or None when fewer than 2 vertices or no edge remain;
    mentions: a new MentionMap — equal (chunk, entity) merged with added weights; RarcUnsupported when a sum reaches 2^12;
    relations: a new RelationList of the rows that stay, in their order — a row is dropped iff its ends were different entities
      of one class, or an end lies outside [0, n); a == b stays — or None when no row stays; relation_rows: the old row of each
      new row (numpy, or a device tensor with as_device=True), for the caller's types and descriptions;
    dropped: {"edges", "edge_weight", "relations_internal", "relations_out_of_range"}.
    ValueError, before any launch, for inputs on different devices or over another number of entities than the plan's."""
    if isinstance(plan_or_labels, MergePlan):
        if richness is not None:
            raise ValueError("richness belongs to merge_plan: a MergePlan has chosen its primaries already")
        plan = plan_or_labels
    else:
        n = _check_labels(plan_or_labels, richness)[0]
        for what, x, k in (("graph", graph, "n"), ("mention map", mentions, "n_entities"), ("relation list", relations, "n_entities")):
            if x is not None and getattr(x, k, n) != n:
                raise ValueError(f"the {what} is over {getattr(x, k)} entities and the labels over {n}: entity i must be label i")
        plan = merge_plan(plan_or_labels, richness, device=_input_device(plan_or_labels, graph, mentions, relations))
    _check_inputs(plan, graph, mentions, relations)
    torch, lib = _require_device()
    dropped = {"edges": 0, "edge_weight": 0, "relations_internal": 0, "relations_out_of_range": 0}
    with torch.cuda.device(plan.device):
        new_graph = None if graph is None else _merge_graph(lib, torch, plan, graph, dropped)
        new_mentions = None if mentions is None else _merge_mentions(lib, torch, plan, mentions)
        new_rel, rows = (None, None) if relations is None else _merge_relations(lib, torch, plan, relations, dropped)
    if rows is not None and not as_device:
        rows = rows.cpu().numpy()
    return MergedEntities(plan, new_graph, new_mentions, new_rel, rows, dropped)


def deduplicate_entities(embeddings, threshold: float = 0.95, richness=None, graph=None, mentions=None, relations=None,
                         max_iterations: int = 10, max_levels: int = 10, device: int = 0, as_device: bool = False,
                         method: str = "louvain") -> MergedEntities:
    """Steps 1-4 of the reference's de-duplication in one call: the pairs of embeddings whose cosine reaches `threshold`, their
    Louvain communities — or with method="components" their connected components, the transitive closure of the pairs — the
    plan and the merge.  The pairs and the labels never leave the device.  Arguments as `entity_clusters` and `merge_entities`
    take them; row i of `embeddings` is entity i."""
    from .communities import _embedding_labels, check_method

    check_method(method)
    n, labels = _embedding_labels(embeddings, threshold, max_iterations, max_levels, device, method)
    if labels is None:
        labels = np.arange(n, dtype=np.int64)                        # nothing was similar: every entity is its own class
    for what, x, k in (("graph", graph, "n"), ("mention map", mentions, "n_entities"), ("relation list", relations, "n_entities")):
        if x is not None and getattr(x, k, n) != n:
            raise ValueError(f"the {what} is over {getattr(x, k)} entities and there are {n} embeddings: row i must be entity i")
    plan = merge_plan(labels, richness, device=device, as_device=as_device)
    return merge_entities(plan, graph=graph, mentions=mentions, relations=relations, as_device=as_device)
