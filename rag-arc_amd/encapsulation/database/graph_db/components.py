"""Connected components of the entity graph, on the MI355X (csrc/components.hip): which entities are joined at all, how many
pieces the graph has and how large they are.

What it replaces: a graph store answers this with

    CALL gds.wcc.stream(graph) YIELD nodeId, componentId

and the reference's fallback de-duplication (encapsulation/database/graph_db/Base_Neo4j.py:922, _fallback_name_based_merge) is a
transitive closure of pairwise matches — the components of the match graph.  Louvain (communities.py) answers another question:
it may cut a chain of near-duplicates in two, and it has max_iterations and max_levels; components are exact, have no parameter,
and their smallest-member labels are what `merge_plan` takes.  Personalized PageRank mass, k-hop levels and shortest paths never
cross a component: `EntityGraph.same_component` says beforehand whether a pair can be joined at all.

`EntityGraph.components()` labels the resident CSR and keeps the answer (the graph is immutable); `connected_components(n, pairs)`
is the one-shot form; `entity_clusters(..., method="components")` and `deduplicate_entities(..., method="components")` take
`similar_pairs`' edge list on the device.

The rule is hook and jump in integers (restated by tests/components_ref.py): the labels, and the number of rounds,
are the same for any order of the edges and from run to run.  The loop over rounds lives here and reads one word per round.  No
CPU fallback: without a device this raises."""
from __future__ import annotations

import collections
import ctypes

import numpy as np

from ....hip import binding as B
from .communities import MAX_EDGES, MAX_VERTICES

ROUND_SLACK = 2                # the additive constant of the round bound (csrc/components.hip)

Components = collections.namedtuple("Components", ("labels", "dense", "sizes", "n_components", "largest", "rounds"))
Components.__doc__ = """labels int64 [n]: the smallest vertex of v's component; dense int32 [n]: the rank of that label among the distinct
labels, ascending; sizes int64 [n_components]: by dense id; largest: (label, size) of the largest component, among equals the smallest
label; rounds: the hook-and-jump rounds taken, the last of which changed nothing (0 for a graph without edges).  numpy arrays, or
device tensors with as_device=True."""


def limits() -> dict:
    """The degree classes of the hook (csrc/components.hip): the largest degree that takes 8 lanes, a quarter wave and the first
    workgroup list, and the additive constant of the round bound."""
    out = (ctypes.c_int * 4)()
    B.check(B.load_library().rarc_components_limits(out), "rarc_components_limits")
    return {"group": out[0], "wave": out[1], "lds": out[2], "round_slack": out[3]}


def round_bound(n: int) -> int:
    """ceil(log2 n) + 2: the rounds every graph met so far stays within, and what the tests hold the kernels to"""
    return max(int(n) - 1, 0).bit_length() + ROUND_SLACK


def round_limit(n: int) -> int:
    """2 ceil(log2 n) + 2: what no graph can exceed (the trees that still have an outside edge at least halve over
    any two rounds, and the last round finds nothing) — past it the loop gives up with a RarcError"""
    return 2 * max(int(n) - 1, 0).bit_length() + ROUND_SLACK


def _run(lib, torch, graph_ptr: int, graph_bytes: int, n: int, m: int, dev, labels_only: bool = False):
    """the rounds and the finish over a CSR blob on `dev` -> Components of device tensors (labels_only: dense and sizes None)"""
    need = int(lib.rarc_components_workspace_bytes(n, m))
    if need == 0:
        raise B.RarcError(f"connected_components: n={n}, m={m} refused by rarc_components_workspace_bytes")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    changed = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    B.check(lib.rarc_components_init(n, m, ws.data_ptr(), ws.numel(), stream), "rarc_components_init")
    # round_limit, not round_bound: a run past ceil(log2 n) + 2 has not been seen but is not excluded (the trees halve over two
    # rounds, not over one), and a legal graph must be answered, not refused; only past the proven limit is something broken
    limit, rounds = round_limit(n), 0
    while True:
        if rounds == limit:
            raise B.RarcError(f"connected_components: still changing after {limit} rounds, more than any graph of n={n} vertices takes")
        B.check(lib.rarc_components_round(graph_ptr, graph_bytes, n, m, ws.data_ptr(), ws.numel(), changed.data_ptr(), stream),
                "rarc_components_round")
        rounds += 1
        if not int(changed.item()):
            break
    labels = torch.empty(n, dtype=torch.int64, device=dev)
    dense = None if labels_only else torch.empty(n, dtype=torch.int32, device=dev)
    sizes = None if labels_only else torch.empty(n, dtype=torch.int64, device=dev)
    out3 = torch.empty(3, dtype=torch.int64, device=dev)
    B.check(lib.rarc_components_finish(n, m, ws.data_ptr(), ws.numel(), labels.data_ptr(), dense.data_ptr() if dense is not None else None,
                                       sizes.data_ptr() if sizes is not None else None, out3.data_ptr(), stream), "rarc_components_finish")
    n_c, size, label = out3.tolist()
    return Components(labels, dense, None if sizes is None else sizes[:n_c], int(n_c), (int(label), int(size)), rounds)


def _host(c: Components) -> Components:
    return Components(c.labels.cpu().numpy(), c.dense.cpu().numpy(), c.sizes.cpu().numpy(), c.n_components, c.largest, c.rounds)


def graph_components(graph, as_device: bool = False) -> Components:
    """EntityGraph.components: computed once per graph, the device and the host form each kept"""
    cache = graph._components
    if True not in cache:
        with graph.torch.cuda.device(graph.device):
            cache[True] = _run(graph.lib, graph.torch, graph._graph.data_ptr(), graph._graph.numel(), graph.n, graph.m, graph.device)
    if not as_device and False not in cache:
        cache[False] = _host(cache[True])
    return cache[bool(as_device)]


def _vertices(graph, x, what: str) -> np.ndarray:
    v = np.asarray(x)
    if v.size and (not np.all(v == np.floor(v)) or v.min() < 0 or v.max() >= graph.n):
        raise ValueError(f"{what} names a vertex outside [0, {graph.n})")
    return v.astype(np.int64)


def component_of(graph, vertices):
    """the label of each vertex's component (the smallest vertex in it): an int for one vertex, else an int64 array of the shape given"""
    v = _vertices(graph, vertices, "component_of")
    out = graph_components(graph).labels[v]
    return int(out) if v.ndim == 0 else out


def same_component(graph, a, b):
    """whether a and b are joined by any path: a bool for two vertices, else a bool array (a and b broadcast)"""
    va, vb = _vertices(graph, a, "same_component"), _vertices(graph, b, "same_component")
    labels = graph_components(graph).labels
    out = labels[va] == labels[vb]
    return bool(out) if np.ndim(out) == 0 else out


def labels_on_device(lib, pairs, n: int, m: int, dev):
    """pairs: device int64 [>= m][2] contiguous, unique (i, j) with 0 <= i < j < n; m >= 1, n >= 2.  -> labels int64 [n] on the
    device, each the smallest member of its component: `_cluster_on_device`'s contract, without its parameters."""
    import torch

    stream = torch.cuda.current_stream(dev).cuda_stream
    graph = torch.empty(int(lib.rarc_graph_csr_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
    B.check(lib.rarc_graph_csr(pairs.data_ptr(), None, None, n, m, graph.data_ptr(), graph.numel(), stream), "rarc_graph_csr")
    return _run(lib, torch, graph.data_ptr(), graph.numel(), n, m, dev, labels_only=True).labels


def _edgeless(n: int, as_device: bool, device: int) -> Components:
    """every vertex its own component: answered without a launch"""
    labels, dense, sizes = np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.int64)
    if as_device:
        import torch

        if not torch.cuda.is_available():
            raise B.RarcError("no ROCm device visible: the HIP backend has no CPU fallback")
        dev = torch.device("cuda", device)
        labels, dense, sizes = (torch.from_numpy(x).to(dev) for x in (labels, dense, sizes))
    return Components(labels, dense, sizes, n, (0, 1) if n else (-1, 0), 0)


def connected_components(n: int, pairs, device: int = 0, as_device: bool = False) -> Components:
    """The connected components of the undirected graph on n vertices whose edges are `pairs` -> Components.
    pairs: an [m][2] array-like — normalised as EntityGraph normalises it: swapped to i < j, duplicates dropped — or an int64
    device tensor [m][2], used where it is: every pair i < j, each once.  ValueError for i == j or an index outside [0, n).
    A graph without edges is answered on the host: every vertex is its own component, in 0 rounds."""
    import torch

    from .pagerank import EntityGraph, _normalise_pairs

    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    on_device = isinstance(pairs, torch.Tensor) and pairs.is_cuda
    if on_device:
        if pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
            raise ValueError(f"expected an int64 [m][2] tensor of pairs, got {pairs.dtype} {tuple(pairs.shape)}")
        m = int(pairs.shape[0])
    else:
        pairs, _ = _normalise_pairs(n, pairs.cpu().numpy() if isinstance(pairs, torch.Tensor) else pairs, None)
        m = int(pairs.shape[0])
    if m >= MAX_EDGES or n >= MAX_VERTICES:
        raise B.RarcUnsupported(f"connected_components(n={n}, {m} edges): the kernels take n < 2^31 - 1 vertices and m < 2^30 edges")
    if m == 0 or n < 2:
        return _edgeless(n, as_device, device)
    return EntityGraph(n, pairs, device=device).components(as_device=as_device)
