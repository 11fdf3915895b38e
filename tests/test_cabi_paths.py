"""The connecting-path exports (rarc_khop_paths, rarc_khop_path_edges, rarc_khop_paths_limits) validate their arguments through the
C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a GPU (the pointers below are
never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes
import types

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
BIG = 1 << 60
N, M, NS, NP, L, R = 1000, 5000, 8, 12, 3, 7000


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _paths(lib, n=N, m=M, ns=NS, np_=NP, length=L, ws=P, wb=BIG, pairs=P, pws=P, pb=BIG, dist=P):
    return lib.rarc_khop_paths(n, m, ns, np_, length, ws, wb, pairs, pws, pb, dist, None)


def _edges(lib, n=N, m=M, nq=NP, hops=L, ws=P, wb=BIG, rel=P, r=R, me=100, ews=P, eb=BIG, ids=P, lv=P, cnt=P, lc=P):
    return lib.rarc_khop_path_edges(n, m, nq, hops, ws, wb, rel, r, me, ews, eb, ids, lv, cnt, lc, None)


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in ("rarc_khop_paths", "rarc_khop_path_edges", "rarc_khop_paths_limits"):
        assert name in B.SIGNATURES and getattr(lib, name)


def test_limits_agree_with_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K

    assert K.paths_limits() == {"max_length": 8, "max_sources": 256, "max_pairs": 256}
    assert (K.MAX_HOPS, K.MAX_PAIRS) == (8, 256) and K.MAX_CONNECT_SEEDS * (K.MAX_CONNECT_SEEDS - 1) // 2 <= 256 < 24 * 23 // 2
    assert B.load_library().rarc_khop_paths_limits(None) == E_INVALID


# ---- rarc_khop_paths ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null", ["ws", "pairs", "pws", "dist"])
def test_paths_null_pointers(null):
    lib = B.load_library()
    assert _paths(lib, **{null: None}) == E_INVALID and b"rarc_khop_paths: null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"ns": 0}, {"ns": -1}, {"ns": 257}, {"np_": 0},
                                {"np_": -1}, {"np_": 257}, {"length": -1}])
def test_paths_shapes_out_of_range(kw):
    lib = B.load_library()
    assert _paths(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert b"rarc_khop_paths:" in lib.rarc_last_error()


def test_paths_longer_than_8_are_unsupported_and_name_the_limit():
    lib = B.load_library()
    assert _paths(lib, length=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error() and b"8" in lib.rarc_last_error()
    assert lib.rarc_khop_workspace_bytes(N, M, NP, 9) == 0                     # the path workspace is a k-hop workspace of np columns
    assert _paths(lib, length=8, wb=0) == E_WORKSPACE and _paths(lib, length=0, wb=0) == E_WORKSPACE


def test_paths_the_limits_themselves_are_accepted_up_to_the_workspace_checks():
    lib = B.load_library()
    for n, m, ns, np_, length in ((2, 1, 1, 1, 0), ((1 << 31) - 2, (1 << 30) - 1, 256, 256, 8), (N, M, 256, 1, 8), (N, M, 1, 256, 0)):
        assert _paths(lib, n=n, m=m, ns=ns, np_=np_, length=length, wb=0) == E_WORKSPACE
        assert _paths(lib, n=n, m=m, ns=ns, np_=np_, length=length, pb=0) == E_WORKSPACE


def test_paths_short_workspaces_each_sized_by_its_own_columns():
    lib = B.load_library()
    need_s, need_p = lib.rarc_khop_workspace_bytes(N, M, 70, L), lib.rarc_khop_workspace_bytes(N, M, 200, L)
    assert 0 < need_s < need_p                                                 # two words of sources, four of pairs
    assert _paths(lib, ns=70, np_=200, wb=need_s - 1, pb=need_p) == E_WORKSPACE and b"rarc_khop_paths: workspace of" in lib.rarc_last_error()
    assert _paths(lib, ns=70, np_=200, wb=need_s, pb=need_p - 1) == E_WORKSPACE and b"path workspace of" in lib.rarc_last_error()
    assert _paths(lib, ns=200, np_=70, wb=need_p, pb=need_s - 1) == E_WORKSPACE and b"path workspace of" in lib.rarc_last_error()
    assert _paths(lib, ns=200, np_=70, wb=need_p - 1, pb=need_s) == E_WORKSPACE and b"rarc_khop_paths: workspace of" in lib.rarc_last_error()


def test_paths_misaligned_pointers():
    lib = B.load_library()
    assert _paths(lib, ws=odd(128)) == E_INVALID and b"the workspace is not 256-byte aligned" in lib.rarc_last_error()
    assert _paths(lib, pws=odd(128)) == E_INVALID and b"path workspace is not 256-byte aligned" in lib.rarc_last_error()
    for kw in ({"pairs": odd(2)}, {"dist": odd(2)}, {"pairs": odd(1)}):
        assert _paths(lib, **kw) == E_INVALID and b"4-byte aligned" in lib.rarc_last_error(), kw
    assert _paths(lib, pairs=odd(4), dist=odd(4), wb=0) == E_WORKSPACE


# ---- rarc_khop_path_edges: the arguments of rarc_khop_edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("null", ["ws", "rel", "ews", "lc"])
def test_edges_null_pointers(null):
    lib = B.load_library()
    assert _edges(lib, **{null: None}) == E_INVALID and b"rarc_khop_path_edges: null pointer" in lib.rarc_last_error()


def test_edges_the_list_outputs_may_be_null_together_and_only_together():
    lib = B.load_library()
    assert _edges(lib, ids=None, lv=None, cnt=None, eb=0) == E_WORKSPACE      # accepted up to the workspace check
    for kw in ({"ids": None}, {"lv": None}, {"cnt": None}, {"ids": None, "lv": None}, {"lv": None, "cnt": None}, {"ids": None, "cnt": None}):
        assert _edges(lib, **kw) == E_INVALID and b"null pointer" in lib.rarc_last_error(), kw


@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nq": 0}, {"nq": -1}, {"nq": 257}, {"hops": -1}])
def test_edges_every_shape_the_traversal_refuses_is_refused(kw):
    lib = B.load_library()
    assert _edges(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert b"rarc_khop_path_edges:" in lib.rarc_last_error()


def test_edges_length_rows_and_the_list_length():
    lib = B.load_library()
    assert _edges(lib, hops=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error() and b"8" in lib.rarc_last_error()
    for r in (0, -1, (1 << 31) - 1, 1 << 40):
        assert _edges(lib, r=r) == E_INVALID and b"relation rows out of range" in lib.rarc_last_error()
    for me in (0, -1):
        assert _edges(lib, me=me) == E_INVALID and b"max_edges" in lib.rarc_last_error()
    assert _edges(lib, me=65537) == E_UNSUPPORTED and b"max_edges=65537" in lib.rarc_last_error() and b"65536" in lib.rarc_last_error()
    assert _edges(lib, me=65536, eb=0) == E_WORKSPACE and _edges(lib, me=1, eb=0) == E_WORKSPACE


def test_edges_short_workspaces_and_misaligned_pointers():
    lib = B.load_library()
    need, eneed = lib.rarc_khop_workspace_bytes(N, M, NP, L), lib.rarc_khop_edges_workspace_bytes(R, NP, L)
    assert _edges(lib, wb=need - 1) == E_WORKSPACE and b"rarc_khop_path_edges: workspace of" in lib.rarc_last_error()
    assert _edges(lib, wb=need, eb=eneed - 1) == E_WORKSPACE and b"edge workspace" in lib.rarc_last_error()
    for n, m, nq, hops, r in ((2, 1, 1, 0, 1), ((1 << 31) - 2, (1 << 30) - 1, 256, 8, (1 << 31) - 2)):
        assert _edges(lib, n=n, m=m, nq=nq, hops=hops, r=r, eb=0) == E_WORKSPACE and _edges(lib, n=n, m=m, nq=nq, hops=hops, r=r, wb=0) == E_WORKSPACE
    assert _edges(lib, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _edges(lib, ews=odd(128)) == E_INVALID and b"edge workspace is not 256-byte aligned" in lib.rarc_last_error()
    for kw in ({"rel": odd(4)}, {"ids": odd(4)}, {"lv": odd(2)}, {"cnt": odd(2)}, {"lc": odd(2)}):
        assert _edges(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), kw


# ---- Python --------------------------------------------------------------------------------------------------------------------------------
def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import RelationList, shortest_paths
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K

    edges = [(0, 1), (1, 2)]
    with pytest.raises(B.RarcUnsupported, match="max_length=9.*8"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)], max_length=9)
    for length in (-1, 1.5):
        with pytest.raises(ValueError, match="max_length"):
            shortest_paths(3, edges, [[0], [2]], [(0, 1)], max_length=length)
    with pytest.raises(B.RarcUnsupported, match="65536"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)], max_vertices=65537)
    with pytest.raises(B.RarcUnsupported, match="65536"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)], max_edges=65537)
    for kw in ({"max_vertices": 0}, {"max_edges": 0}, {"max_vertices": None}):
        with pytest.raises(ValueError):
            shortest_paths(3, edges, [[0], [2]], [(0, 1)], **kw)
    for sources in ([[3]], [[-2]], [], [list(range(3)) * 22]):                 # outside [0, n), no sources, 66 seeds
        with pytest.raises(ValueError):
            shortest_paths(3, edges, sources, [(0, 0)])
    for pairs in ([(0, 2)], [(-1, 0)], [], [(0, 1, 1)], [0, 1], [(0.5, 1)]):   # outside [0, ns), none, not [np][2], no integers
        with pytest.raises(ValueError):
            shortest_paths(3, edges, [[0], [2]], pairs)
    with pytest.raises(B.RarcUnsupported, match="257 sources.*256"):
        shortest_paths(3, edges, [[0]] * 257, [(0, 1)])
    with pytest.raises(B.RarcUnsupported, match="257 pairs.*256"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)] * 257)
    with pytest.raises(ValueError, match="RelationList"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)], relations=edges)
    rel = RelationList.__new__(RelationList)
    rel.n_entities, rel.device = 4, "cuda:0"
    with pytest.raises(ValueError, match="RelationList"):
        shortest_paths(3, edges, [[0], [2]], [(0, 1)], relations=rel)
    assert K.host_pairs(2, [(0, 1), (1, 1)]).dtype == np.int32 and K.check_length(0) == 0 and K.check_length(8) == 8
    # the methods check in the same order: nothing of the graph is touched before the arguments are refused
    graph = types.SimpleNamespace(n=3, device="cuda:0")
    with pytest.raises(B.RarcUnsupported, match="max_length=9"):
        K.shortest_paths(graph, [[0]], [(0, 0)], max_length=9)
    with pytest.raises(B.RarcUnsupported, match="max_length=9"):
        K.path_chunks(graph, None, [[0]], [(0, 0)], max_length=9)
    with pytest.raises(ValueError, match="decay"):
        K.path_chunks(graph, None, [[0]], [(0, 0)], max_length=2, decay=[1, 2])
    with pytest.raises(ValueError, match="MentionMap"):
        K.path_chunks(graph, None, [[0]], [(0, 0)], max_length=2)
    with pytest.raises(B.RarcUnsupported, match="max_length=9"):
        K.connect(graph, None, None, max_length=9)
    index = types.SimpleNamespace(ntotal=3)
    graph._check_index = lambda index, k: None
    with pytest.raises(ValueError, match="at least 2"):
        K.connect(graph, index, None, seeds_per_query=1)
    with pytest.raises(B.RarcUnsupported, match="seeds_per_query=24.*276 pairs"):
        K.connect(graph, index, None, seeds_per_query=24)


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import shortest_paths

    if torch.cuda.is_available():
        got = shortest_paths(3, [(0, 1), (1, 2)], [[0], [2]], [(0, 1)], max_length=2, max_vertices=4, max_edges=4)
        assert got.distances.tolist() == [2] and got.vertex_ids.tolist() == [[0, 1, 2, -1]] and got.edge_level_counts.tolist() == [[0, 1, 1]]
        return
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        shortest_paths(3, [(0, 1), (1, 2)], [[0], [2]], [(0, 1)])
