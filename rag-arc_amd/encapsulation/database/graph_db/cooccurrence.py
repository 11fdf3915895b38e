"""The co-occurrence projection of a mention map, on the MI355X (csrc/cooccur.hip): two entities are joined when a chunk mentions
both, weighted by how many chunks do.

What it replaces: the reference stores `(chunk)-[:MENTIONS]->(entity)` (event_graphrag_neo4j.py:508-557) and a HippoRAG-style or
local-search retriever walks the projection of those links,

    MATCH (a:Entity)<-[:MENTIONS]-(c:Chunk)-[:MENTIONS]->(b:Entity) WHERE id(a) < id(b)
    RETURN a, b, count(c) AS weight

the pattern under gds.graph.project.cypher and gds.nodeSimilarity.  Without it the caller pulls the mention list to the host,
forms the upper triangle of AᵀA in scipy.sparse and pushes the pairs back; here `MentionMap` is resident already, the pairs are
expanded, sorted (rarc_sort_reduce) and summed next to it, and `EntityGraph.from_device` adopts them: from mentions to ranked chunks
no edge list crosses to the host and no extracted relation table is needed.

    mm = MentionMap(n_chunks, n_entities, mentions)
    graph = mm.cooccurrence()                                  # an EntityGraph
    graph.rank_chunks(mm, seeds, top_k=10)

After a merge the contracted map implies another projection, taken the same way:

    merged = merge_entities(labels, mentions=mm)
    graph = merged.mentions.cooccurrence()

The rule is in integers (restated by tests/cooccur_ref.py): the edges and weights are the same bits for any order
of the mentions, for either weight form, and from run to run.  No CPU fallback: without a device this raises."""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from ....hip import binding as B
from .merge import MAX_COUNT

MIN_MAX_MENTIONS = 2
MAX_MAX_MENTIONS = 4096        # the row of a workgroup in LDS (csrc/cooccur.hip)
MAX_EDGE_WEIGHT = 1 << 32      # W is returned as uint32
WEIGHTS = {"count": 0, "product": 1}

Cooccurrence = collections.namedtuple("Cooccurrence", ("pairs", "weights", "total_pairs", "chunks_skipped", "largest_weight"))
Cooccurrence.__doc__ = """pairs int64 [m][2]: the edges (a, b), a < b, by (a, b) ascending; weights uint32 [m]: W(a, b) (a device tensor
holds the bits as int32); total_pairs: T, the pairs expanded before equal ones were summed; chunks_skipped: the chunks of more than
max_mentions mentions, which gave nothing; largest_weight: the largest W, edges below min_weight included.  numpy arrays, or device
tensors with as_device=True."""


def limits() -> dict:
    """The constants of the expansion (csrc/cooccur.hip): the most mentions a single wave expands (a chunk of more takes a
    workgroup), the largest max_mentions, the bits of a product value and the limit of T."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_cooccur_limits(out), "rarc_cooccur_limits")
    return {"wave_degree": out[0], "max_mentions": out[1], "product_bits": out[2], "max_total_pairs": 1 << out[3]}


def check_arguments(n_entities: int, weight, min_weight, max_mentions):
    """-> (mode, min_weight, max_mentions) as integers; ValueError for what the rule does not take"""
    if weight not in WEIGHTS:
        raise ValueError(f"weight must be 'count' or 'product', got {weight!r}")
    if isinstance(min_weight, bool) or min_weight != int(min_weight) or int(min_weight) < 1:
        raise ValueError(f"min_weight must be an integer >= 1, got {min_weight!r}")
    if isinstance(max_mentions, bool) or max_mentions != int(max_mentions) or not MIN_MAX_MENTIONS <= int(max_mentions) <= MAX_MAX_MENTIONS:
        raise ValueError(f"max_mentions must lie in [{MIN_MAX_MENTIONS}, {MAX_MAX_MENTIONS}], got {max_mentions!r}")
    if int(n_entities) < 2:
        raise ValueError("a co-occurrence graph needs at least 2 entities")
    return WEIGHTS[weight], int(min_weight), int(max_mentions)


def _empty(torch, dev, as_device: bool):
    if as_device:
        return torch.empty((0, 2), dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    return np.zeros((0, 2), np.int64), np.zeros(0, np.uint32)


def cooccurrence_pairs(mentions, weight: str = "count", min_weight: int = 1, max_mentions: int = 64, as_device: bool = False) -> Cooccurrence:
    """The edges of the co-occurrence projection of `mentions` (a MentionMap) -> Cooccurrence.
    A chunk of 2 .. max_mentions mentions gives every two of its entities a < b the value 1 (weight="count") or w_a * w_b
    (weight="product"); a chunk of more gives nothing and is counted (one chunk of 4096 mentions is 8.4 M pairs).  W(a, b) is the
    sum over all chunks; an edge exists iff W >= min_weight.  No edge at all is a valid, empty answer.
    ValueError, before the device is needed, for another weight form, min_weight < 1, max_mentions outside [2, 4096] or fewer than
    2 entities; RarcUnsupported when the pairs to expand reach 2^31 (a smaller max_mentions leaves out the hubs that cause it) or
    a W reaches 2^32 (weight="product" only)."""
    from .passages import MentionMap

    if not isinstance(mentions, MentionMap):
        raise ValueError("mentions must be a MentionMap")
    mode, min_weight, max_mentions = check_arguments(mentions.n_entities, weight, min_weight, max_mentions)
    torch, lib, dev = mentions.torch, mentions.lib, mentions.device
    nc, nnz, n = mentions.n_chunks, mentions.nnz, mentions.n_entities
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        need = int(lib.rarc_cooccur_workspace_bytes(nc, nnz))
        if need == 0:
            raise B.RarcError(f"cooccurrence_pairs: n_chunks={nc}, nnz={nnz} refused by rarc_cooccur_workspace_bytes")
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out4 = torch.empty(4, dtype=torch.int64, device=dev)
        csr = (mentions._row_ptr.data_ptr(), mentions._ent.data_ptr(), mentions._w.data_ptr(), nc, nnz, n)
        B.check(lib.rarc_cooccur_count(*csr, max_mentions, ws.data_ptr(), ws.numel(), out4.data_ptr(), stream), "rarc_cooccur_count")
        total, _, over, _ = out4.tolist()                               # (entries outside the rule are skipped, as the rule says)
        if total >= MAX_COUNT:
            raise B.RarcUnsupported(f"the co-occurrence of this map expands to T = {total} pairs: rarc_sort_reduce takes T < 2^31; a smaller "
                                    f"max_mentions (now {max_mentions}) leaves out the chunks that mention most")
        if total == 0:
            return Cooccurrence(*_empty(torch, dev, as_device), 0, int(over), 0)
        keys = torch.empty(total, dtype=torch.int64, device=dev)
        values = torch.empty(total, dtype=torch.int32, device=dev) if mode else None
        B.check(lib.rarc_cooccur_emit(*csr, mode, ws.data_ptr(), ws.numel(), keys.data_ptr(), values.data_ptr() if mode else None, total, stream),
                "rarc_cooccur_emit")
        del ws
        sws = torch.empty(int(lib.rarc_sort_reduce_workspace_bytes(total)), dtype=torch.uint8, device=dev)
        ukeys, sums = torch.empty(total, dtype=torch.int64, device=dev), torch.empty(total, dtype=torch.int64, device=dev)
        out2 = torch.empty(2, dtype=torch.int64, device=dev)
        key_bits = 2 * max(1, (n - 1).bit_length())
        B.check(lib.rarc_sort_reduce(keys.data_ptr(), values.data_ptr() if mode else None, total, key_bits, sws.data_ptr(), sws.numel(),
                                     ukeys.data_ptr(), sums.data_ptr(), out2.data_ptr(), stream), "rarc_sort_reduce")
        distinct = int(out2[0].item())
        del sws, keys, values
        ews = torch.empty(int(lib.rarc_cooccur_edges_workspace_bytes(distinct)), dtype=torch.uint8, device=dev)
        pairs = torch.empty((distinct, 2), dtype=torch.int64, device=dev)
        w = torch.empty(distinct, dtype=torch.int32, device=dev)
        out3 = torch.empty(3, dtype=torch.int64, device=dev)
        B.check(lib.rarc_cooccur_edges(ukeys.data_ptr(), sums.data_ptr(), distinct, n, min_weight, ews.data_ptr(), ews.numel(), pairs.data_ptr(),
                                       w.data_ptr(), out3.data_ptr(), stream), "rarc_cooccur_edges")
        m, largest, _ = out3.tolist()
        largest &= (1 << 64) - 1
        if largest >= MAX_EDGE_WEIGHT:
            raise B.RarcUnsupported(f"the weights of a co-occurrence edge add up to {largest}: an edge weight must stay below 2^32")
        pairs, w = pairs[:m], w[:m]
        if not as_device:
            pairs, w = pairs.cpu().numpy(), w.cpu().numpy().view(np.uint32)
        return Cooccurrence(pairs, w, int(total), int(over), int(largest))


def cooccurrence(mentions, weight: str = "count", min_weight: int = 1, max_mentions: int = 64):
    """MentionMap.cooccurrence: the projection as an EntityGraph over the map's entities, built where the pairs lie.
    ValueError("no two entities share a chunk") when there is no edge; the refusals of cooccurrence_pairs, and those of
    EntityGraph.from_device (a total weight of 2^31 or more among them)."""
    from .pagerank import EntityGraph

    got = cooccurrence_pairs(mentions, weight=weight, min_weight=min_weight, max_mentions=max_mentions, as_device=True)
    if int(got.pairs.shape[0]) == 0:
        raise ValueError("no two entities share a chunk")
    return EntityGraph.from_device(mentions.n_entities, got.pairs, got.weights)


def cooccurrence_graph(n_chunks: int, n_entities: int, mentions, weights=None, device: int = 0, **kw):
    """The one-call form: MentionMap(n_chunks, n_entities, mentions, weights, device).cooccurrence(**kw)."""
    from .passages import MentionMap

    check_arguments(n_entities, kw.get("weight", "count"), kw.get("min_weight", 1), kw.get("max_mentions", 64))
    return MentionMap(n_chunks, n_entities, mentions, weights=weights, device=device).cooccurrence(**kw)
