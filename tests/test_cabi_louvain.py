"""The Louvain exports (rarc_graph_csr, rarc_louvain_init / _sweep / _aggregate / _labels and their workspace sizes) validate their
arguments through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a GPU
(the pointers below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 50
N, M = 1000, 5000


def _csr(lib, pairs=P, w=None, loops=None, n=N, m=M, graph=P, gb=BIG):
    return lib.rarc_graph_csr(pairs, w, loops, n, m, graph, gb, None)


def _init(lib, graph=P, gb=BIG, n=N, m=M, state=P, sb=BIG, out=P):
    return lib.rarc_louvain_init(graph, gb, n, m, state, sb, out, None)


def _sweep(lib, graph=P, gb=BIG, n=N, m=M, state=P, sb=BIG, cur=0, sweep=0, out=P):
    return lib.rarc_louvain_sweep(graph, gb, n, m, state, sb, cur, sweep, out, None)


def _agg(lib, graph=P, gb=BIG, n=N, m=M, state=P, sb=BIG, cur=0, labels=P, n0=N, pairs=P, w=P, loops=P, counts=P):
    return lib.rarc_louvain_aggregate(graph, gb, n, m, state, sb, cur, labels, n0, pairs, w, loops, counts, None)


def _labels(lib, labels=P, n0=N, ws=P, wb=BIG):
    return lib.rarc_louvain_labels(labels, n0, ws, wb, None)


CALLS = {"csr": _csr, "init": _init, "sweep": _sweep, "aggregate": _agg, "labels": _labels}


def test_version_is_unchanged():
    assert B.load_library().rarc_version() == 600


@pytest.mark.parametrize("call,null", [("csr", "pairs"), ("csr", "graph"), ("init", "graph"), ("init", "state"), ("init", "out"),
                                       ("sweep", "graph"), ("sweep", "state"), ("sweep", "out"), ("aggregate", "graph"),
                                       ("aggregate", "state"), ("aggregate", "labels"), ("aggregate", "pairs"), ("aggregate", "w"),
                                       ("aggregate", "loops"), ("aggregate", "counts"), ("labels", "labels"), ("labels", "ws")])
def test_null_pointers(call, null):
    lib = B.load_library()
    assert CALLS[call](lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()
    assert call.encode() in lib.rarc_last_error()


def test_weights_and_loops_may_be_null():
    """level 0 has neither: the call gets as far as the workspace check"""
    lib = B.load_library()
    assert _csr(lib, w=None, loops=None, gb=0) == E_WORKSPACE


@pytest.mark.parametrize("call", ["csr", "init", "sweep", "aggregate"])
@pytest.mark.parametrize("kw", [{"n": 1}, {"n": 0}, {"n": -1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": -3}, {"m": 1 << 30}])
def test_n_and_m_out_of_range(call, kw):
    lib = B.load_library()
    if call == "aggregate" and "n" in kw:
        kw = dict(kw, n0=max(kw["n"], 2))
    assert CALLS[call](lib, **kw) == E_INVALID
    assert b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for n, m in ((2, 1), ((1 << 31) - 2, 1), (N, (1 << 30) - 1)):
        assert lib.rarc_graph_csr_workspace_bytes(n, m) > 0 and lib.rarc_louvain_workspace_bytes(n, m) > 0
        assert _csr(lib, n=n, m=m, gb=0) == E_WORKSPACE and _sweep(lib, n=n, m=m, gb=0) == E_WORKSPACE


def test_short_workspaces():
    lib = B.load_library()
    gneed, sneed = lib.rarc_graph_csr_workspace_bytes(N, M), lib.rarc_louvain_workspace_bytes(N, M)
    # the adjacency in both directions (neighbour, weight, source: 3 x 4 bytes x 2 m), row pointers, four lists of vertices
    assert gneed >= 24 * M + 8 * (N + 1) + 16 * N
    # two slots of (label, tot, size) and the pair table of the aggregate (12 bytes x at least 2 m slots)
    assert sneed >= 24 * N + 24 * M
    assert _csr(lib, gb=gneed - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error()
    for call in (_init, _sweep, _agg):
        assert call(lib, gb=gneed - 1, sb=sneed) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
        assert call(lib, gb=gneed, sb=sneed - 1) == E_WORKSPACE and b"state workspace" in lib.rarc_last_error()
    lneed = lib.rarc_louvain_labels_workspace_bytes(N)
    assert lneed >= 4 * N
    assert _labels(lib, wb=lneed - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error()
    assert lib.rarc_graph_csr_workspace_bytes(N, 2 * M) > gneed and lib.rarc_louvain_workspace_bytes(2 * N, M) > sneed


@pytest.mark.parametrize("args", [(1, 5), (0, 5), (-1, 5), ((1 << 31) - 1, 5), (N, 0), (N, -1), (N, 1 << 30)])
def test_workspace_bytes_is_zero_on_bad_arguments(args):
    lib = B.load_library()
    assert lib.rarc_graph_csr_workspace_bytes(*args) == 0 and lib.rarc_louvain_workspace_bytes(*args) == 0


def test_sweep_index_slot_and_label_count():
    lib = B.load_library()
    assert _sweep(lib, sweep=-1) == E_INVALID and b"sweep index -1" in lib.rarc_last_error()
    assert _sweep(lib, cur=2) == E_INVALID and b"slot" in lib.rarc_last_error()
    assert _agg(lib, cur=-1) == E_INVALID and b"slot" in lib.rarc_last_error()
    assert _agg(lib, n0=N - 1) == E_INVALID and b"n0" in lib.rarc_last_error()
    for n0 in (0, -1, (1 << 31) - 1):
        assert _labels(lib, n0=n0) == E_INVALID and b"out of range" in lib.rarc_last_error()
        assert lib.rarc_louvain_labels_workspace_bytes(n0) == 0
    assert _sweep(lib, sweep=1 << 20, gb=0) == E_WORKSPACE          # any sweep index >= 0 passes: only its low bits select


def test_bucket_limits():
    from rag_arc_amd.encapsulation.database.graph_db import communities

    lim = communities.bucket_limits()
    assert 1 <= lim["group"] < lim["wave"] == 64 < lim["lds"] and lim["lds_slots"] >= 2 * lim["lds"]
    assert lim["lds_slots"] * 8 + 64 <= 160 * 1024                  # the table fits a CU's LDS
    assert B.load_library().rarc_louvain_limits(None) == E_INVALID


def test_python_surface_refuses_before_it_needs_a_device():
    from rag_arc_amd.encapsulation.database.graph_db import entity_clusters, louvain_communities

    for n, pairs in ((3, [(1, 1)]), (3, [(0, 3)]), (3, [(-1, 2)]), (3, [(0, 1, 2)])):
        with pytest.raises(ValueError):
            louvain_communities(n, pairs)
    for kw in ({"max_iterations": 0}, {"max_levels": 0}):
        with pytest.raises(ValueError):
            louvain_communities(3, [(0, 1)], **kw)
        with pytest.raises(ValueError):
            louvain_communities(3, [], **kw)
        with pytest.raises(ValueError):
            entity_clusters([[1.0, 0.0], [0.0, 1.0]], **kw)
    for kw in ({"threshold": 0.0}, {"threshold": 1.5}, {"min_size": 0}):
        with pytest.raises(ValueError):
            entity_clusters([[1.0, 0.0], [0.0, 1.0]], **kw)
    with pytest.raises(B.RarcUnsupported, match="2\\^31"):
        louvain_communities((1 << 31) - 1, [(0, 1)])


def test_nothing_to_cluster_needs_no_device():
    import numpy as np

    from rag_arc_amd.encapsulation.database.graph_db import louvain_communities

    for n, pairs in ((5, []), (5, np.zeros((0, 2), np.int64)), (1, []), (0, [])):
        got = louvain_communities(n, pairs)
        assert got.dtype == np.int64 and np.array_equal(got, np.arange(n))


def test_clusters_of_orders_by_size_then_smallest_member():
    from rag_arc_amd.encapsulation.database.graph_db.communities import clusters_of

    labels = [0, 1, 2, 1, 0, 5, 2, 1, 8]
    assert clusters_of(labels) == [[1, 3, 7], [0, 4], [2, 6]]
    assert clusters_of(labels, min_size=1) == [[1, 3, 7], [0, 4], [2, 6], [5], [8]]
    assert clusters_of(labels, min_size=3) == [[1, 3, 7]] and clusters_of([], 1) == []


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rag_arc_amd.encapsulation.database.graph_db import entity_clusters, louvain_communities

    with pytest.raises(B.RarcError, match="no CPU fallback"):
        louvain_communities(3, [(0, 1)])
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        entity_clusters([[1.0, 0.0], [0.0, 1.0]])
