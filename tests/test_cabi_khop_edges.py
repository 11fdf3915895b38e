"""The k-hop subgraph exports (rarc_khop_edges, its workspace size and limits) validate their arguments through the C-ABI before
anything touches a device: error codes with a rarc_last_error text on a box without a GPU (the pointers below are never
dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes
import types

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
BIG = 1 << 60
N, M, NQ, HOPS, R = 1000, 5000, 8, 3, 7000


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _edges(lib, n=N, m=M, nq=NQ, hops=HOPS, ws=P, wb=BIG, rel=P, r=R, me=100, ews=P, eb=BIG, ids=P, lv=P, cnt=P, lc=P):
    return lib.rarc_khop_edges(n, m, nq, hops, ws, wb, rel, r, me, ews, eb, ids, lv, cnt, lc, None)


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in ("rarc_khop_edges", "rarc_khop_edges_workspace_bytes", "rarc_khop_edges_limits"):
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("null", ["ws", "rel", "ews", "lc"])
def test_null_pointers(null):
    lib = B.load_library()
    assert _edges(lib, **{null: None}) == E_INVALID and b"rarc_khop_edges: null pointer" in lib.rarc_last_error()


def test_the_list_outputs_may_be_null_together_and_only_together():
    lib = B.load_library()
    assert _edges(lib, ids=None, lv=None, cnt=None, eb=0) == E_WORKSPACE      # accepted up to the workspace check
    for kw in ({"ids": None}, {"lv": None}, {"cnt": None}, {"ids": None, "lv": None}, {"lv": None, "cnt": None}, {"ids": None, "cnt": None}):
        assert _edges(lib, **kw) == E_INVALID and b"null pointer" in lib.rarc_last_error(), kw


@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nq": 0}, {"nq": -1}, {"nq": 257}, {"hops": -1}])
def test_every_shape_the_traversal_refuses_is_refused(kw):
    lib = B.load_library()
    assert _edges(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert b"rarc_khop_edges:" in lib.rarc_last_error()
    if "n" not in kw and "m" not in kw:                                      # (the edge workspace does not depend on n and m)
        assert lib.rarc_khop_edges_workspace_bytes(R, kw.get("nq", NQ), kw.get("hops", HOPS)) == 0


def test_more_than_8_hops_is_unsupported_and_names_the_limit():
    lib = B.load_library()
    assert _edges(lib, hops=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error() and b"8" in lib.rarc_last_error()
    assert lib.rarc_khop_edges_workspace_bytes(R, NQ, 9) == 0 and lib.rarc_khop_edges_workspace_bytes(R, NQ, 8) > 0


def test_the_rows_and_the_list_length():
    lib = B.load_library()
    for r in (0, -1, (1 << 31) - 1, 1 << 40):
        assert _edges(lib, r=r) == E_INVALID and b"relation rows out of range" in lib.rarc_last_error()
        assert lib.rarc_khop_edges_workspace_bytes(r, NQ, HOPS) == 0
    for me in (0, -1):
        assert _edges(lib, me=me) == E_INVALID and b"max_edges" in lib.rarc_last_error()
    assert _edges(lib, me=65537) == E_UNSUPPORTED and b"max_edges=65537" in lib.rarc_last_error() and b"65536" in lib.rarc_last_error()
    assert _edges(lib, me=65536, eb=0) == E_WORKSPACE and _edges(lib, me=1, eb=0) == E_WORKSPACE


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for n, m, nq, hops, r in ((2, 1, 1, 0, 1), ((1 << 31) - 2, (1 << 30) - 1, 256, 8, (1 << 31) - 2), (N, M, 256, 8, R), (N, M, 64, 0, 1)):
        assert lib.rarc_khop_edges_workspace_bytes(r, nq, hops) > 0
        assert _edges(lib, n=n, m=m, nq=nq, hops=hops, r=r, eb=0) == E_WORKSPACE
        assert _edges(lib, n=n, m=m, nq=nq, hops=hops, r=r, wb=0) == E_WORKSPACE


def test_short_workspaces_and_the_size_of_the_edge_workspace():
    lib = B.load_library()
    need = lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS)
    assert _edges(lib, wb=need - 1) == E_WORKSPACE and b"workspace of" in lib.rarc_last_error()
    eneed = lib.rarc_khop_edges_workspace_bytes(R, NQ, HOPS)
    tiles = (R + 1023) // 1024
    assert eneed >= tiles * (HOPS + 1) * 64 * 4                               # one count per (tile, level, query of the word)
    assert lib.rarc_khop_edges_workspace_bytes(R, 64, HOPS) == eneed < lib.rarc_khop_edges_workspace_bytes(R, 65, HOPS)
    assert lib.rarc_khop_edges_workspace_bytes(R, NQ, HOPS + 1) > eneed and lib.rarc_khop_edges_workspace_bytes(8 * R, NQ, HOPS) > eneed
    assert _edges(lib, wb=need, eb=eneed - 1) == E_WORKSPACE and b"edge workspace" in lib.rarc_last_error()
    assert lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS) == need              # (the traversal's workspace is what it was)


def test_misaligned_pointers():
    lib = B.load_library()
    assert _edges(lib, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _edges(lib, ews=odd(128)) == E_INVALID and b"edge workspace is not 256-byte aligned" in lib.rarc_last_error()
    for kw in ({"rel": odd(4)}, {"ids": odd(4)}, {"lv": odd(2)}, {"cnt": odd(2)}, {"lc": odd(2)}):
        assert _edges(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), kw
    assert _edges(lib, rel=odd(8), ids=odd(8), lv=odd(4), cnt=odd(4), lc=odd(4), eb=0) == E_WORKSPACE


def test_limits_agree_with_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K

    assert K.edges_limits() == {"max_edges": K.MAX_LIST_EDGES, "tile": 1024} and K.MAX_LIST_EDGES == 65536
    assert B.load_library().rarc_khop_edges_limits(None) == E_INVALID


def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import RelationList, k_hop_subgraph
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K

    pairs = [(0, 1), (1, 2)]
    with pytest.raises(B.RarcUnsupported, match="65536"):
        k_hop_subgraph(3, pairs, [[0]], max_edges=65537)
    for me in (0, -1, 1.5):
        with pytest.raises(ValueError, match="max_edges"):
            k_hop_subgraph(3, pairs, [[0]], max_edges=me)
    with pytest.raises(B.RarcUnsupported, match="65536"):
        k_hop_subgraph(3, pairs, [[0]], max_vertices=65537)
    with pytest.raises(B.RarcUnsupported, match="hops=9.*8"):
        k_hop_subgraph(3, pairs, [[0]], hops=9)
    for seeds in ([[3]], [[-2]], []):
        with pytest.raises(ValueError):
            k_hop_subgraph(3, pairs, seeds)
    for bad in ([], [[0, 1, 2]], [0, 1], [[0.0, 1.0]], [[[0, 1]]], np.zeros((0, 2), np.int64)):   # empty, not [r][2], no integers
        with pytest.raises(ValueError):
            RelationList(3, bad)
    for bad in ([], [[0, 1, 2]], [0, 1], [[0.5, 1.0]], [[0, 3]], [[1, 1]]):                      # the graph's own pairs, as EntityGraph checks them
        with pytest.raises(ValueError):
            k_hop_subgraph(3, bad, [[0]])
    with pytest.raises(ValueError, match="weights"):
        RelationList(3, pairs, weights=[1.0])
    with pytest.raises(ValueError, match="RelationList"):
        k_hop_subgraph(3, pairs, [[0]], relations=pairs)
    # a list over another n_entities, or on another device: refused against the graph it is used with
    graph = types.SimpleNamespace(n=3, device="cuda:0")
    rel = RelationList.__new__(RelationList)
    rel.n_entities, rel.device = 4, "cuda:0"
    with pytest.raises(ValueError, match="4 entities"):
        K.check_relations(graph, rel)
    with pytest.raises(ValueError, match="RelationList"):
        k_hop_subgraph(3, pairs, [[0]], relations=rel)
    rel.n_entities, rel.device = 3, "cuda:1"
    with pytest.raises(ValueError, match="cuda:1"):
        K.check_relations(graph, rel)
    with pytest.raises(ValueError, match="RelationList"):
        K.check_relations(graph, pairs)
    rel.device = "cuda:0"
    K.check_relations(graph, rel)
    K.check_relations(graph, None)
    assert K.check_max_edges(1) == 1 and K.check_max_edges(65536) == 65536


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import RelationList, k_hop_subgraph

    if torch.cuda.is_available():
        got = k_hop_subgraph(3, [(0, 1), (1, 2)], [[0]], hops=1)
        assert got.edge_ids[0, :got.edge_counts[0]].tolist() == [0] and got.edge_level_counts.tolist() == [[0, 1]]
        return
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        k_hop_subgraph(3, [(0, 1), (1, 2)], [[0]], hops=1)
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        RelationList(3, [(0, 1), (1, 2)])
