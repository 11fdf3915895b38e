"""The two embedding self-joins of the reference's graph store, on the MI355X: all pairs of embeddings whose cosine reaches a
threshold (csrc/pairs.hip, `rarc_similar_pairs`) and every embedding's exact top-K cosine neighbours (csrc/knn.hip,
`rarc_knn_graph`: `knn_graph` below).

What it replaces in the reference (encapsulation/database/graph_db/Base_Neo4j.py:559-583):

    embeddings_array = np.array(embeddings)
    similarity_matrix = cosine_similarity(embeddings_array)          # sklearn: n x n float64
    for i in range(len(embeddings)):
        for j in range(i + 1, len(embeddings)):
            if similarity_matrix[i][j] >= similarity_threshold:      # 0.95
                ... CREATE (e1)-[:SIMILAR {similarity: float(similarity_matrix[i][j])}]->(e2)

`similar_pairs(embeddings, 0.95)` returns those (i, j, similarity) triples in that loop's order.  The matrix is never formed
(the score GEMM nominates, an exact double-precision pass decides), so 100,000 entities cost tens of milliseconds instead of
80 GB of float64 and 5e9 interpreter steps.  No CPU fallback: without the HIP library this raises."""
from __future__ import annotations

import ctypes
from typing import List, Tuple

import numpy as np

from ....hip import binding as B

MAX_DIM = 4096
MAX_TOP_K = 256      # csrc/knn.hip: KNN_KMAX


def _pairs_on_device(lib, x, threshold: float, dev):
    """rarc_similar_pairs' launch-and-regrow loop on contiguous fp32 rows [n >= 2][d] of `dev` (the current device):
    (pairs int64 [cap][2], cosines float64 [cap], found) — device tensors whose first `found` entries are the pairs, in no
    particular order.  `similar_pairs` copies them to the host; `entity_clusters` clusters them where they are."""
    import torch

    n, d = int(x.shape[0]), int(x.shape[1])
    cand_cap, out_cap = 256, max(1024, 4 * n)
    n_pad = (n + 255) // 256 * 256
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    while True:
        ws = torch.empty(int(lib.rarc_similar_pairs_workspace_bytes(n, d, cand_cap)), dtype=torch.uint8, device=dev)
        pairs = torch.empty((out_cap, 2), dtype=torch.int64, device=dev)
        scores = torch.empty(out_cap, dtype=torch.float64, device=dev)
        B.check(lib.rarc_similar_pairs(x.data_ptr(), x.stride(0), n, d, ctypes.c_double(threshold), ws.data_ptr(),
                                       ws.numel(), cand_cap, pairs.data_ptr(), scores.data_ptr(), out_cap, count.data_ptr(),
                                       flags.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "rarc_similar_pairs")
        f, found = int(flags.item()), int(count.item())
        if f == 0:
            return pairs, scores, found
        if f & 1:
            if cand_cap >= n_pad:
                raise B.RarcError("rarc_similar_pairs flagged a nomination list that holds every row")
            cand_cap = min(4 * cand_cap, n_pad)
        if f & 2:
            out_cap = max(found, 2 * out_cap)       # (an overflowed list hid nominations: the count may still grow)


def similar_pairs(embeddings, threshold: float = 0.95, device: int = 0, as_arrays: bool = False):
    """[(i, j, cosine)] for every i < j with cosine(embeddings[i], embeddings[j]) >= threshold, ordered by (i, j).
    embeddings: [n][d] array-like of floats (the reference holds python lists) or a torch tensor (used where it is).
    as_arrays=True returns (pairs int64 [m][2], cosines float64 [m]) instead — half a million pairs are 0.1 s of python
    objects otherwise."""
    import torch

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
                return (np.zeros((0, 2), np.int64), np.zeros(0, np.float64)) if as_arrays else []
            raise ValueError(f"expected [n][d] embeddings, got an array of shape {arr.shape}")
        x = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if x.ndim != 2:
        raise ValueError(f"expected [n][d] embeddings, got a tensor of shape {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 2:
        return (np.zeros((0, 2), np.int64), np.zeros(0, np.float64)) if as_arrays else []
    if not 1 <= d <= MAX_DIM:
        raise B.RarcError(f"embeddings of {d} dimensions: the all-pairs kernel takes 1..{MAX_DIM}")
    if not 0.0 < float(threshold) <= 1.0:
        raise ValueError("threshold must lie in (0, 1]")
    with torch.cuda.device(dev):
        pairs, scores, found = _pairs_on_device(lib, x.contiguous(), float(threshold), dev)
        p = pairs[:found].cpu().numpy()
        s = scores[:found].cpu().numpy()
    order = np.lexsort((p[:, 1], p[:, 0]))
    p, s = p[order], s[order]
    if as_arrays:
        return p, s
    return list(zip(p[:, 0].tolist(), p[:, 1].tolist(), s.tolist()))


def _knn_empty(n: int, top_k: int, as_arrays: bool):
    if as_arrays:
        return np.full((n, top_k), -1, np.int64), np.full((n, top_k), -np.inf, np.float64), np.zeros(n, np.int32)
    return []


def knn_graph(embeddings, top_k: int = 10, similarity_cutoff: float = 0.0, device: int = 0, as_arrays: bool = False):
    """Every embedding's top_k other embeddings by cosine, exactly: [(i, j, cosine)] for each row i and each of its neighbours
    j != i with cosine >= similarity_cutoff, ordered by (i asc, cosine desc, j asc) — the directed SIMILAR_TO edges
    `gds.knn.write` writes in the reference (event_graphrag_neo4j.py:636-649 passes topK 10, similarityCutoff 0.85; the
    defaults here are GDS's own).  Scores are raw float64 cosines in [-1, 1], the ones `similar_pairs` returns for the same
    pair; the answer is exact where GDS's NN-descent is approximate.  Self is excluded by index: an identical copy of row i is
    its neighbour.
    embeddings: [n][d] array-like of floats or a torch tensor (used where it is).
    as_arrays=True returns (neighbours int64 [n][top_k], cosines float64 [n][top_k], counts int32 [n]) instead, padded with
    (-1, -inf) past each row's count."""
    import math

    import torch

    top_k = int(top_k)
    cutoff = float(similarity_cutoff)
    if top_k < 1:
        raise ValueError("top_k must be at least 1")
    if not (math.isfinite(cutoff) and -1.0 <= cutoff <= 1.0):
        raise ValueError("similarity_cutoff must lie in [-1, 1]")
    if top_k > MAX_TOP_K:
        raise B.RarcUnsupported(f"knn_graph(top_k={top_k}): the kNN kernel keeps at most top_k = {MAX_TOP_K} neighbours per row "
                                f"(csrc/knn.hip); for a threshold rather than a count, similar_pairs answers without a limit")
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
                return _knn_empty(0, top_k, as_arrays)
            raise ValueError(f"expected [n][d] embeddings, got an array of shape {arr.shape}")
        x = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
    if x.ndim != 2:
        raise ValueError(f"expected [n][d] embeddings, got a tensor of shape {tuple(x.shape)}")
    n, d = int(x.shape[0]), int(x.shape[1])
    if n < 2:
        return _knn_empty(n, top_k, as_arrays)
    if not 1 <= d <= MAX_DIM:
        raise B.RarcError(f"embeddings of {d} dimensions: the kNN kernel takes 1..{MAX_DIM}")
    x = x.contiguous()
    n_pad = (n + 255) // 256 * 256
    # A column's list holds what the first chunk of rows nominates, then K plus a margin.  Under a cutoff that random rows
    # reach (<= 0: half of them or all) that is the whole first chunk; under a selective one only near-duplicates get in.
    first = (max(512, 2 * (top_k + 1)) + 255) // 256 * 256
    cand_cap = min(n_pad, first + 256 if cutoff <= 0.0 else max(64, 4 * top_k))
    ids = torch.empty((n, top_k), dtype=torch.int64, device=dev)
    cos = torch.empty((n, top_k), dtype=torch.float64, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        while True:
            ws = torch.empty(int(lib.rarc_knn_graph_workspace_bytes(n, d, top_k, cand_cap)), dtype=torch.uint8, device=dev)
            B.check(lib.rarc_knn_graph(x.data_ptr(), x.stride(0), n, d, top_k, ctypes.c_double(cutoff), ws.data_ptr(), ws.numel(),
                                       cand_cap, ids.data_ptr(), cos.data_ptr(), counts.data_ptr(), flags.data_ptr(),
                                       torch.cuda.current_stream(dev).cuda_stream), "rarc_knn_graph")
            if int(flags.item()) == 0:
                break
            if cand_cap >= n_pad:
                raise B.RarcError("rarc_knn_graph flagged a nomination list that holds every row")
            del ws
            cand_cap = min(4 * cand_cap, n_pad)
        nb, cs, ct = ids.cpu().numpy(), cos.cpu().numpy(), counts.cpu().numpy()
    if as_arrays:
        return nb, cs, ct
    have = nb >= 0                                   # row-major: (i asc, then the row's own order)
    src = np.nonzero(have)[0]
    return list(zip(src.tolist(), nb[have].tolist(), cs[have].tolist()))
