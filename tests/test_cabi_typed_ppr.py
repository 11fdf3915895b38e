"""The typed-PageRank exports (rarc_graph_types_weighted and its workspace size, rarc_ppr_seed_typed, rarc_ppr_step_typed; DESIGN
§4.13m) validate their arguments through the C-ABI before anything touches a device: error codes with a rarc_last_error text on
a box without a GPU (the pointers below are never dereferenced)."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 60
N, M, NQ, S = 1000, 5000, 8, 5
NAMES = ("rarc_graph_types_weighted_workspace_bytes", "rarc_graph_types_weighted", "rarc_ppr_seed_typed", "rarc_ppr_step_typed")


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _tb(lib, n=N, m=M):
    return lib.rarc_graph_types_weighted_workspace_bytes(n, m)


def _types(lib, graph=P, gb=BIG, n=N, m=M, pairs=P, masks=P, weights=P, out=P, ob=BIG):
    return lib.rarc_graph_types_weighted(graph, gb, n, m, pairs, masks, weights, out, ob, None)


def _seed(lib, graph=P, gb=BIG, ty=P, tb=None, filters=P, n=N, m=M, seeds=P, w=P, nq=NQ, s=S, ws=P, wb=BIG):
    return lib.rarc_ppr_seed_typed(graph, gb, ty, _tb(lib, n, m) if tb is None else tb, filters, n, m, seeds, w, nq, s, ws, wb, None)


def _step(lib, graph=P, gb=BIG, ty=P, tb=None, filters=P, n=N, m=M, nq=NQ, a=55706, tol=0, cur=0, ws=P, wb=BIG, done=None):
    return lib.rarc_ppr_step_typed(graph, gb, ty, _tb(lib, n, m) if tb is None else tb, filters, n, m, nq, a, tol, cur, ws, wb, done, None)


ENTRIES = {"rarc_ppr_seed_typed": _seed, "rarc_ppr_step_typed": _step}


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in NAMES:
        assert name in B.SIGNATURES and getattr(lib, name)


# ---- rarc_graph_types_weighted -------------------------------------------------------------------------------------------------------
def _align(b):
    return (b + 255) & ~255


@pytest.mark.parametrize("n,m", [(N, M), (2, 1), (1000, 33), (77, 4097), ((1 << 31) - 2, (1 << 30) - 1)])
def test_the_weighted_size_is_the_unweighted_size_and_the_weight_plane(n, m):
    lib = B.load_library()
    plain = lib.rarc_graph_types_workspace_bytes(n, m)
    assert plain > 0 and plain % 256 == 0
    assert lib.rarc_graph_types_weighted_workspace_bytes(n, m) == plain + _align(2 * m * 4)


@pytest.mark.parametrize("null", ["graph", "pairs", "masks", "out"])
def test_graph_types_weighted_null_pointers(null):
    lib = B.load_library()
    assert _types(lib, **{null: None}) == E_INVALID and b"rarc_graph_types_weighted: null pointer" in lib.rarc_last_error()


def test_graph_types_weighted_shapes_sizes_and_alignment():
    lib = B.load_library()
    for kw in ({"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}):
        assert _types(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error()
        assert b"rarc_graph_types_weighted:" in lib.rarc_last_error()
        assert lib.rarc_graph_types_weighted_workspace_bytes(kw.get("n", N), kw.get("m", M)) == 0
    need = _tb(lib)
    assert _types(lib, ob=need - 1) == E_WORKSPACE and b"typed adjacency of" in lib.rarc_last_error()
    assert _types(lib, ob=lib.rarc_graph_types_workspace_bytes(N, M)) == E_WORKSPACE            # the unweighted size is too small
    assert _types(lib, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    for kw in ({"graph": odd(128)}, {"out": odd(128)}):
        assert _types(lib, **kw) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error(), kw
    for kw in ({"pairs": odd(4)}, {"masks": odd(2)}, {"weights": odd(2)}):
        assert _types(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), kw
    # null weights are unit weights: every other check is passed and the size refuses
    assert _types(lib, weights=None, ob=0) == E_WORKSPACE
    assert _types(lib, pairs=odd(8), masks=odd(4), weights=odd(4), ob=0) == E_WORKSPACE


def test_the_unweighted_entry_is_what_it_was():
    lib = B.load_library()
    assert lib.rarc_graph_types(None, BIG, N, M, P, P, P, BIG, None) == E_INVALID and b"rarc_graph_types: null pointer" in lib.rarc_last_error()
    assert lib.rarc_graph_types(P, BIG, N, M, P, odd(2), P, BIG, None) == E_INVALID
    assert b"rarc_graph_types: an array is not aligned to its element (pairs 8 bytes, masks 4)" in lib.rarc_last_error()
    need = lib.rarc_graph_types_workspace_bytes(N, M)
    assert lib.rarc_graph_types(P, BIG, N, M, P, P, P, need - 1, None) == E_WORKSPACE
    assert b"rarc_graph_types: typed adjacency of %d bytes, %d needed" % (need - 1, need) in lib.rarc_last_error()


# ---- rarc_ppr_seed_typed, rarc_ppr_step_typed ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,null", [("rarc_ppr_seed_typed", x) for x in ("graph", "ty", "filters", "seeds", "w", "ws")]
                         + [("rarc_ppr_step_typed", x) for x in ("graph", "ty", "filters", "ws")])
def test_null_pointers(entry, null):
    lib = B.load_library()
    assert ENTRIES[entry](lib, **{null: None}) == E_INVALID and entry.encode() + b": null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_misaligned_types_and_filters(entry):
    lib = B.load_library()
    for a in (4, 128):
        assert ENTRIES[entry](lib, ty=odd(a)) == E_INVALID and entry.encode() + b": the typed adjacency is not 256-byte aligned" in lib.rarc_last_error()
    for a in (1, 2):
        assert ENTRIES[entry](lib, filters=odd(a)) == E_INVALID and entry.encode() + b": the filters are not 4-byte aligned" in lib.rarc_last_error()
    assert ENTRIES[entry](lib, filters=odd(4), wb=0) == E_WORKSPACE


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_types_bytes_other_than_the_weighted_size(entry):
    lib = B.load_library()
    need = _tb(lib)
    for tb in (0, lib.rarc_graph_types_workspace_bytes(N, M), need - 1, need + 1, need + 256, BIG):
        assert ENTRIES[entry](lib, tb=tb) == E_WORKSPACE, tb
        msg = lib.rarc_last_error()
        assert entry.encode() + b": typed adjacency of %d bytes" % tb in msg and b"%d" % need in msg and b"rarc_graph_types_weighted" in msg
    # the right size passes this check: the next one, the workspace, refuses
    assert ENTRIES[entry](lib, tb=need, wb=lib.rarc_ppr_workspace_bytes(N, M, NQ) - 1) == E_WORKSPACE
    assert entry.encode() + b": workspace of" in lib.rarc_last_error()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nq": 0}, {"nq": -1}, {"nq": 257}])
def test_every_shape_the_untyped_entries_refuse(entry, kw):
    lib = B.load_library()
    assert lib.rarc_ppr_workspace_bytes(kw.get("n", N), kw.get("m", M), kw.get("nq", NQ)) == 0
    assert ENTRIES[entry](lib, tb=BIG, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert entry.encode() + b":" in lib.rarc_last_error()


def test_the_limits_themselves_are_accepted_and_the_rest_of_the_arguments_checked():
    lib = B.load_library()
    for n, m, nq in ((2, 1, 1), ((1 << 31) - 2, (1 << 30) - 1, 256), (N, M, 65)):
        assert _seed(lib, n=n, m=m, nq=nq, wb=0) == E_WORKSPACE and _step(lib, n=n, m=m, nq=nq, wb=0) == E_WORKSPACE
    assert _seed(lib, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    assert _step(lib, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    for s in (0, -1, 65):
        assert _seed(lib, s=s) == E_INVALID and b"%d seed slots out of range" % s in lib.rarc_last_error()
    for a in (-1, 65536):
        assert _step(lib, a=a) == E_INVALID and b"damping" in lib.rarc_last_error()
    for tol in (-1, (1 << 40) + 1):
        assert _step(lib, tol=tol) == E_INVALID and b"tolerance" in lib.rarc_last_error()
    for cur in (-1, 2):
        assert _step(lib, cur=cur) == E_INVALID and b"slot %d is neither 0 nor 1" % cur in lib.rarc_last_error()
