"""The typed-traversal exports (rarc_graph_types and its workspace size, rarc_khop_step_typed, rarc_khop_edges_typed,
rarc_khop_path_edges_typed) validate their arguments through the C-ABI before anything touches a device: error
codes with a rarc_last_error text on a box without a GPU (the pointers below are never dereferenced)."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
BIG = 1 << 60
N, M, NQ, HOPS, R = 1000, 5000, 8, 3, 7000
NAMES = ("rarc_graph_types_workspace_bytes", "rarc_graph_types", "rarc_khop_step_typed", "rarc_khop_edges_typed", "rarc_khop_path_edges_typed")
ROW_ENTRIES = ("rarc_khop_edges_typed", "rarc_khop_path_edges_typed")


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _types(lib, graph=P, gb=BIG, n=N, m=M, pairs=P, masks=P, out=P, ob=BIG):
    return lib.rarc_graph_types(graph, gb, n, m, pairs, masks, out, ob, None)


def _step(lib, graph=P, gb=BIG, ty=P, tb=BIG, filters=P, n=N, m=M, nq=NQ, hops=HOPS, hop=1, ws=P, wb=BIG, grew=None):
    return lib.rarc_khop_step_typed(graph, gb, ty, tb, filters, n, m, nq, hops, hop, ws, wb, grew, None)


def _rows(lib, entry, n=N, m=M, nq=NQ, hops=HOPS, ws=P, wb=BIG, rel=P, r=R, rt=P, rm=0, filters=P, me=100, ews=P, eb=BIG, ids=P, lv=P, cnt=P,
          lc=P):
    return getattr(lib, entry)(n, m, nq, hops, ws, wb, rel, r, rt, rm, filters, me, ews, eb, ids, lv, cnt, lc, None)


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in NAMES:
        assert name in B.SIGNATURES and getattr(lib, name)


# ---- rarc_graph_types ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null", ["graph", "pairs", "masks", "out"])
def test_graph_types_null_pointers(null):
    lib = B.load_library()
    assert _types(lib, **{null: None}) == E_INVALID and b"rarc_graph_types: null pointer" in lib.rarc_last_error()


def test_graph_types_shapes_sizes_and_alignment():
    lib = B.load_library()
    for kw in ({"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}):
        assert _types(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error()
        assert lib.rarc_graph_types_workspace_bytes(kw.get("n", N), kw.get("m", M)) == 0
    need = lib.rarc_graph_types_workspace_bytes(N, M)
    assert need >= 2 * M * 4 + 2 * M * 4 + N * 4 + 4                       # t_adj | t_mask | cursor | the bad-pair count
    assert lib.rarc_graph_types_workspace_bytes(N, 2 * M) > need and lib.rarc_graph_types_workspace_bytes(2 * N, M) > need
    assert _types(lib, ob=need - 1) == E_WORKSPACE and b"typed adjacency of" in lib.rarc_last_error()
    assert _types(lib, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    for kw in ({"graph": odd(128)}, {"out": odd(128)}):
        assert _types(lib, **kw) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error(), kw
    for kw in ({"pairs": odd(4)}, {"masks": odd(2)}):
        assert _types(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), kw
    assert _types(lib, pairs=odd(8), masks=odd(4), ob=0) == E_WORKSPACE
    for n, m in ((2, 1), ((1 << 31) - 2, (1 << 30) - 1)):                  # the limits themselves are accepted
        assert lib.rarc_graph_types_workspace_bytes(n, m) > 0 and _types(lib, n=n, m=m, ob=0) == E_WORKSPACE


# ---- rarc_khop_step_typed ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null", ["graph", "ty", "filters", "ws"])
def test_step_null_pointers(null):
    lib = B.load_library()
    assert _step(lib, **{null: None}) == E_INVALID and b"rarc_khop_step_typed: null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nq": 0}, {"nq": -1}, {"nq": 257}, {"hops": -1}])
def test_step_refuses_every_shape_the_untyped_step_refuses(kw):
    lib = B.load_library()
    assert _step(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert b"rarc_khop_step_typed:" in lib.rarc_last_error()


def test_step_hops_hop_sizes_and_alignment():
    lib = B.load_library()
    assert _step(lib, hops=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error() and b"8" in lib.rarc_last_error()
    for hop in (0, -1, HOPS + 1):
        assert _step(lib, hop=hop) == E_INVALID and b"hop %d out of range" % hop in lib.rarc_last_error()
    assert _step(lib, hops=0, hop=1) == E_INVALID
    assert _step(lib, hop=HOPS, wb=0) == E_WORKSPACE
    need = lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS)
    assert _step(lib, wb=need - 1) == E_WORKSPACE and b"workspace of" in lib.rarc_last_error()
    assert _step(lib, wb=need, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    assert _step(lib, wb=need, tb=lib.rarc_graph_types_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"typed adjacency" in lib.rarc_last_error()
    assert _step(lib, graph=odd(128)) == E_INVALID and b"graph is not 256-byte aligned" in lib.rarc_last_error()
    assert _step(lib, ty=odd(128)) == E_INVALID and b"typed adjacency is not 256-byte aligned" in lib.rarc_last_error()
    assert _step(lib, ws=odd(128)) == E_INVALID and b"workspace is not 256-byte aligned" in lib.rarc_last_error()
    for kw in ({"filters": odd(2)}, {"grew": odd(2)}):
        assert _step(lib, **kw) == E_INVALID and b"4-byte aligned" in lib.rarc_last_error(), kw
    assert _step(lib, filters=odd(4), grew=odd(4), wb=0) == E_WORKSPACE
    for n, m, nq, hops in ((2, 1, 1, 1), ((1 << 31) - 2, (1 << 30) - 1, 256, 8), (N, M, 65, 8)):
        assert _step(lib, n=n, m=m, nq=nq, hops=hops, hop=hops, wb=0) == E_WORKSPACE


# ---- rarc_khop_edges_typed, rarc_khop_path_edges_typed -----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ROW_ENTRIES)
@pytest.mark.parametrize("null", ["ws", "rel", "rt", "filters", "ews", "lc"])
def test_rows_null_pointers(entry, null):
    lib = B.load_library()
    assert _rows(lib, entry, **{null: None}) == E_INVALID and entry.encode() + b": null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("entry", ROW_ENTRIES)
def test_rows_list_outputs_may_be_null_together_and_only_together(entry):
    lib = B.load_library()
    assert _rows(lib, entry, ids=None, lv=None, cnt=None, eb=0) == E_WORKSPACE
    for kw in ({"ids": None}, {"lv": None}, {"cnt": None}, {"ids": None, "lv": None}, {"lv": None, "cnt": None}, {"ids": None, "cnt": None}):
        assert _rows(lib, entry, **kw) == E_INVALID and b"null pointer" in lib.rarc_last_error(), kw


@pytest.mark.parametrize("entry", ROW_ENTRIES)
@pytest.mark.parametrize("kw", [{"n": 1}, {"m": 1 << 30}, {"nq": 0}, {"nq": 257}, {"hops": -1}, {"r": 0}, {"r": (1 << 31) - 1}, {"me": 0}, {"rm": 2},
                                {"rm": -1}])
def test_rows_refuse_what_the_untyped_entries_refuse_and_a_bad_mask_flag(entry, kw):
    lib = B.load_library()
    assert _rows(lib, entry, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert entry.encode() + b":" in lib.rarc_last_error()


@pytest.mark.parametrize("entry", ROW_ENTRIES)
def test_rows_limits_sizes_and_alignment(entry):
    lib = B.load_library()
    assert _rows(lib, entry, hops=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error()
    assert _rows(lib, entry, me=65537) == E_UNSUPPORTED and b"max_edges=65537" in lib.rarc_last_error() and b"65536" in lib.rarc_last_error()
    need, eneed = lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS), lib.rarc_khop_edges_workspace_bytes(R, NQ, HOPS)
    assert _rows(lib, entry, wb=need - 1) == E_WORKSPACE and b"workspace of" in lib.rarc_last_error()
    assert _rows(lib, entry, wb=need, eb=eneed - 1) == E_WORKSPACE and b"edge workspace" in lib.rarc_last_error()
    for rm in (0, 1):
        assert _rows(lib, entry, rm=rm, me=65536, eb=0) == E_WORKSPACE
    assert _rows(lib, entry, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _rows(lib, entry, ews=odd(128)) == E_INVALID and b"edge workspace is not 256-byte aligned" in lib.rarc_last_error()
    for kw in ({"rt": odd(2)}, {"filters": odd(2)}):
        assert _rows(lib, entry, **kw) == E_INVALID and b"row types or the filters are not 4-byte aligned" in lib.rarc_last_error(), kw
    for kw in ({"rel": odd(4)}, {"ids": odd(4)}, {"lv": odd(2)}, {"cnt": odd(2)}, {"lc": odd(2)}):
        assert _rows(lib, entry, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), kw
    assert _rows(lib, entry, rel=odd(8), rt=odd(4), filters=odd(4), ids=odd(8), lv=odd(4), cnt=odd(4), lc=odd(4), eb=0) == E_WORKSPACE
    for n, m, nq, hops, r in ((2, 1, 1, 0, 1), ((1 << 31) - 2, (1 << 30) - 1, 256, 8, (1 << 31) - 2)):
        assert _rows(lib, entry, n=n, m=m, nq=nq, hops=hops, r=r, eb=0) == E_WORKSPACE


def test_the_untyped_workspaces_are_what_they_were():
    lib = B.load_library()
    assert lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS) == lib.rarc_khop_workspace_bytes(N, M, 64, HOPS)
    tiles = (R + 1023) // 1024
    assert lib.rarc_khop_edges_workspace_bytes(R, NQ, HOPS) >= tiles * (HOPS + 1) * 64 * 4
