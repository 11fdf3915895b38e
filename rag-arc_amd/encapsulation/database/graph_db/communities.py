"""Louvain communities of the similarity graph, on the MI355X (csrc/louvain.hip): steps 2 and 3 of the reference's entity
de-duplication (encapsulation/database/graph_db/Base_Neo4j.py:646-658).

What it replaces in the reference:

    CALL gds.louvain.stream(graph, {maxIterations: 10}) YIELD nodeId, communityId
    WITH communityId, collect(nodeId) AS nodeIds WHERE size(nodeIds) > 1
    RETURN communityId, nodeIds ORDER BY size(nodeIds) DESC

which needs a Neo4j server with the GDS plugin (without it the reference falls back to merging by name, :392-395).
`entity_clusters(embeddings)` answers it from the embeddings alone: `rarc_similar_pairs` leaves the SIMILAR edges on the device
and the Louvain kernels cluster them there; only the labels leave HBM.  `louvain_communities(n, pairs)` clusters any edge list.

GDS's Louvain is parallel and order-dependent; this one is defined in integers (restated by
tests/louvain_ref.py) and returns the same labels for any order of the edges.  The loops over sweeps and levels live here and
read three words per sweep.  No CPU fallback: without the HIP library this raises."""
from __future__ import annotations

import ctypes
from typing import List

import numpy as np

from ....hip import binding as B
from . import similarity as S

MAX_EDGES = 1 << 30            # csrc/louvain.hip: m < 2^30 and n < 2^31 - 1 keep every product of the rule inside int64
MAX_VERTICES = (1 << 31) - 1
METHODS = ("louvain", "components")


def check_method(method) -> str:
    """ValueError for anything but "louvain" or "components": raised before anything else is looked at"""
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    return method


def bucket_limits() -> dict:
    """The degree classes of the sweep (csrc/louvain.hip): the largest degree that takes the 8-lane form, the wave form and the
    LDS-table form, and that table's slots; a vertex of a larger degree takes the global-memory table."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_louvain_limits(out), "rarc_louvain_limits")
    return {"group": out[0], "wave": out[1], "lds": out[2], "lds_slots": out[3]}


def _check_counts(n: int, m: int, max_iterations: int, max_levels: int) -> None:
    if max_iterations < 1 or max_levels < 1:
        raise ValueError("max_iterations and max_levels must be at least 1")
    if n < 0:
        raise ValueError("n must not be negative")
    if m >= MAX_EDGES or n >= MAX_VERTICES:
        raise B.RarcUnsupported(f"louvain_communities(n={n}, {m} edges): the kernels take n < 2^31 - 1 vertices and m < 2^30 edges "
                                "(the integer gains fit int64 below that)")


def _cluster_on_device(lib, pairs, n: int, m: int, max_iterations: int, max_levels: int, dev):
    """pairs: device int64 [>= m][2] contiguous, unique (i, j) with 0 <= i < j < n; m >= 1, n >= 2.  -> labels int64 [n] on the
    device, each the smallest member of its community."""
    import torch

    stream = torch.cuda.current_stream(dev).cuda_stream
    graph = torch.empty(int(lib.rarc_graph_csr_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
    state = torch.empty(int(lib.rarc_louvain_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
    labels = torch.arange(n, dtype=torch.int64, device=dev)
    out2 = torch.zeros(3, dtype=torch.int64, device=dev)
    nxt_pairs = torch.empty((m, 2), dtype=torch.int64, device=dev)
    nxt_w = torch.empty(m, dtype=torch.int32, device=dev)
    nxt_loops = torch.empty(n, dtype=torch.int32, device=dev)
    g, gb, s, sb = graph.data_ptr(), graph.numel(), state.data_ptr(), state.numel()
    n_l, m_l = n, m
    edges, weights, loops = pairs, None, None
    for level in range(max_levels):
        B.check(lib.rarc_graph_csr(edges.data_ptr(), weights.data_ptr() if weights is not None else None,
                                   loops.data_ptr() if loops is not None else None, n_l, m_l, g, gb, stream), "rarc_graph_csr")
        B.check(lib.rarc_louvain_init(g, gb, n_l, m_l, s, sb, out2.data_ptr(), stream), "rarc_louvain_init")
        best = int(out2[1].item())
        cur, idle = 0, 0
        for t in range(max_iterations):
            B.check(lib.rarc_louvain_sweep(g, gb, n_l, m_l, s, sb, cur, t, out2.data_ptr(), stream), "rarc_louvain_sweep")
            moved, q, targets = out2.tolist()
            if moved == 0:                      # nothing changed: no Qn to test.  Idle if no mover had a target (two idle
                idle = idle + 1 if targets == 0 else 0      # sweeps in a row end the level); movers the singleton rule
                if idle == 2:                               # held back wait for a sweep in which their target moves
                    break
                continue
            idle = 0
            if q <= best:                       # the sweep overshot: it is discarded (slot `cur` still holds the labels)
                break
            best, cur = q, cur ^ 1
        # the aggregate writes the next level's edges into buffers the current level's CSR does not read (it has its own copy)
        B.check(lib.rarc_louvain_aggregate(g, gb, n_l, m_l, s, sb, cur, labels.data_ptr(), n, nxt_pairs.data_ptr(), nxt_w.data_ptr(),
                                           nxt_loops.data_ptr(), out2.data_ptr(), stream), "rarc_louvain_aggregate")
        n_c, m_c = out2[:2].tolist()
        if n_c == n_l or m_c == 0 or n_c < 2:   # nothing merged, or nothing left that could
            break
        n_l, m_l = int(n_c), int(m_c)
        edges, weights, loops = nxt_pairs, nxt_w, nxt_loops
    ws = torch.empty(int(lib.rarc_louvain_labels_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    B.check(lib.rarc_louvain_labels(labels.data_ptr(), n, ws.data_ptr(), ws.numel(), stream), "rarc_louvain_labels")
    return labels


def louvain_communities(n: int, pairs, max_iterations: int = 10, max_levels: int = 10, device: int = 0) -> np.ndarray:
    """labels int64 [n]: labels[v] = the smallest vertex of v's community, for the undirected unit-weight graph on n vertices
    whose edges are `pairs`.
    pairs: an [m][2] array-like — normalised here: swapped to i < j, duplicates dropped — or an int64 device tensor [m][2],
    used where it is: every pair i < j, each once.  ValueError for i == j or an index outside [0, n).
    max_iterations: sweeps per level (the reference passes maxIterations: 10); max_levels: GDS's default 10."""
    import torch

    n, max_iterations, max_levels = int(n), int(max_iterations), int(max_levels)
    on_device = isinstance(pairs, torch.Tensor) and pairs.is_cuda
    if on_device:
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
            raise ValueError(f"expected an int64 [m][2] tensor of pairs, got {pairs.dtype} {tuple(pairs.shape)}")
        m = int(pairs.shape[0])
        _check_counts(n, m, max_iterations, max_levels)
        if m and not bool(((pairs[:, 0] >= 0) & (pairs[:, 0] < pairs[:, 1]) & (pairs[:, 1] < n)).all().item()):
            raise ValueError(f"device pairs must satisfy 0 <= i < j < {n}")
    else:
        arr = np.asarray(pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs)
        if arr.size == 0:
            arr = np.zeros((0, 2), np.int64)
        if arr.ndim != 2 or arr.shape[1] != 2:
            raise ValueError(f"expected [m][2] pairs, got an array of shape {arr.shape}")
        if not np.issubdtype(arr.dtype, np.integer):
            if not np.all(arr == np.floor(arr)):
                raise ValueError("pairs must be integers")
        arr = arr.astype(np.int64)
        if arr.shape[0]:
            if arr.min() < 0 or arr.max() >= n:
                raise ValueError(f"a pair names a vertex outside [0, {n})")
            if np.any(arr[:, 0] == arr[:, 1]):
                raise ValueError("a pair (i, i): self-loops are not part of the input")
            arr = np.unique(np.stack([arr.min(axis=1), arr.max(axis=1)], axis=1), axis=0)
        m = int(arr.shape[0])
        _check_counts(n, m, max_iterations, max_levels)
    if m == 0 or n <= 1:
        return np.arange(n, dtype=np.int64)
    if not torch.cuda.is_available():
        raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
    lib = B.load_library()
    dev = torch.device("cuda", device)
    with torch.cuda.device(dev):
        p = pairs.to(dev).contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        return _cluster_on_device(lib, p, n, m, max_iterations, max_levels, dev).cpu().numpy()


def clusters_of(labels: np.ndarray, min_size: int = 2) -> List[List[int]]:
    """The communities of at least min_size members as ascending lists of indices, ordered by size descending, then by smallest
    member ascending (the reference's WHERE size(nodeIds) > 1 ... ORDER BY size(nodeIds) DESC)."""
    labels = np.asarray(labels, dtype=np.int64)
    order = np.argsort(labels, kind="stable")            # members of a community together, each run ascending
    uniq, start, count = np.unique(labels[order], return_index=True, return_counts=True)
    keep = np.nonzero(count >= min_size)[0]
    keep = keep[np.lexsort((uniq[keep], -count[keep]))]  # a label IS the smallest member
    return [order[start[i]:start[i] + count[i]].tolist() for i in keep]


def entity_clusters(embeddings, threshold: float = 0.95, max_iterations: int = 10, max_levels: int = 10, min_size: int = 2,
                    device: int = 0, as_labels: bool = False, method: str = "louvain"):
    """The Louvain communities of the graph that joins every two embeddings whose cosine reaches `threshold`: lists of row
    indices, each ascending, only those of at least min_size rows, ordered by size descending and then by smallest member.
    as_labels=True returns labels int64 [n] instead (labels[i] = the smallest row of i's community).
    embeddings: [n][d] array-like of floats or a torch tensor (used where it is).  The pairs never leave the device.
    method="components" clusters by the connected components of that graph instead (graph_db/components.py): the rows that are
    transitively near-duplicates, exact and without parameters — max_iterations and max_levels are checked and not used."""
    check_method(method)
    min_size = int(min_size)
    if int(max_iterations) >= 1 and int(max_levels) >= 1 and min_size < 1:
        raise ValueError("min_size must be at least 1")
    n, labels = _embedding_labels(embeddings, threshold, max_iterations, max_levels, device, method)
    labels = np.arange(n, dtype=np.int64) if labels is None else labels.cpu().numpy()
    return labels if as_labels else clusters_of(labels, min_size)


def _embedding_labels(embeddings, threshold, max_iterations, max_levels, device, method="louvain"):
    """entity_clusters up to the labels -> (n, labels int64 [n] on the device, or None where nothing was clustered: fewer than 2
    rows, or no pair reached the threshold); `deduplicate_entities` goes on from them where they are"""
    import torch

    max_iterations, max_levels = int(max_iterations), int(max_levels)
    if max_iterations < 1 or max_levels < 1:
        raise ValueError("max_iterations and max_levels must be at least 1")
    if not 0.0 < float(threshold) <= 1.0:
        raise ValueError("threshold must lie in (0, 1]")
    if not torch.cuda.is_available():
        raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
    lib = B.load_library()
    dev = torch.device("cuda", device)
    if isinstance(embeddings, torch.Tensor):
        x = embeddings.to(device=dev, dtype=torch.float32)
    else:
        arr = np.asarray(embeddings, dtype=np.float32)
        if arr.ndim != 2:
            if arr.size == 0:
                return 0, None
            raise ValueError(f"expected [n][d] embeddings, got an array of shape {arr.shape}")
        x = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if x.ndim != 2:
        raise ValueError(f"expected [n][d] embeddings, got a tensor of shape {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n >= 2 and not 1 <= d <= S.MAX_DIM:
        raise B.RarcError(f"embeddings of {d} dimensions: the all-pairs kernel takes 1..{S.MAX_DIM}")
    if n >= 2:
        with torch.cuda.device(dev):
            pairs, _, found = S._pairs_on_device(lib, x.contiguous(), float(threshold), dev)
            _check_counts(n, found, max_iterations, max_levels)
            if found and method == "components":
                from .components import labels_on_device

                return n, labels_on_device(lib, pairs, n, found, dev)
            if found:
                return n, _cluster_on_device(lib, pairs, n, found, max_iterations, max_levels, dev)
    return n, None
