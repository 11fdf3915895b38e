"""The connected-components exports (rarc_components_init / _round / _finish, their workspace size and limits) validate their
arguments through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a GPU (the
pointers below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 60
N, M = 1000, 5000


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _init(lib, n=N, m=M, ws=P, wb=BIG):
    return lib.rarc_components_init(n, m, ws, wb, None)


def _round(lib, graph=P, gb=BIG, n=N, m=M, ws=P, wb=BIG, changed=P):
    return lib.rarc_components_round(graph, gb, n, m, ws, wb, changed, None)


def _finish(lib, n=N, m=M, ws=P, wb=BIG, labels=P, dense=P, sizes=P, out3=P):
    return lib.rarc_components_finish(n, m, ws, wb, labels, dense, sizes, out3, None)


CALLS = {"rarc_components_init": _init, "rarc_components_round": _round, "rarc_components_finish": _finish}


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in list(CALLS) + ["rarc_components_workspace_bytes", "rarc_components_limits"]:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("call,null", [("rarc_components_init", "ws"), ("rarc_components_round", "graph"), ("rarc_components_round", "ws"),
                                       ("rarc_components_round", "changed"), ("rarc_components_finish", "ws"),
                                       ("rarc_components_finish", "labels"), ("rarc_components_finish", "out3")])
def test_null_pointers(call, null):
    lib = B.load_library()
    assert CALLS[call](lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()


def test_the_dense_ids_and_the_sizes_may_be_null():
    lib = B.load_library()
    for kw in ({"dense": None}, {"sizes": None}, {"dense": None, "sizes": None}):
        assert _finish(lib, wb=0, **kw) == E_WORKSPACE                      # accepted up to the workspace check


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("kw", [{"n": 1}, {"n": 0}, {"n": -3}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": -1}, {"m": 1 << 30}])
def test_shapes_out_of_range(call, kw):
    lib = B.load_library()
    assert CALLS[call](lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()
    assert lib.rarc_components_workspace_bytes(kw.get("n", N), kw.get("m", M)) == 0


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for n, m in ((2, 1), ((1 << 31) - 2, (1 << 30) - 1), (N, M)):
        assert lib.rarc_components_workspace_bytes(n, m) > 0
        for name, call in CALLS.items():
            assert call(lib, n=n, m=m, wb=0) == E_WORKSPACE, name


def test_short_workspaces():
    lib = B.load_library()
    need = lib.rarc_components_workspace_bytes(N, M)
    assert need >= 4 * N * 4                                                 # two parent arrays, the sizes and the ranks
    assert lib.rarc_components_workspace_bytes(N, 1) == need                 # the state is per vertex
    assert lib.rarc_components_workspace_bytes(2 * N, M) > need
    for name, call in CALLS.items():
        assert call(lib, wb=need - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error(), name
        assert name.encode() + b":" in lib.rarc_last_error()
    gneed = lib.rarc_graph_csr_workspace_bytes(N, M)
    assert _round(lib, wb=need, gb=gneed - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()


def test_misaligned_pointers():
    lib = B.load_library()
    for name, call in CALLS.items():
        assert call(lib, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error(), name
    assert _round(lib, graph=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _round(lib, changed=odd(2)) == E_INVALID and b"4-byte aligned" in lib.rarc_last_error()
    for kw in ({"labels": odd(4)}, {"dense": odd(2)}, {"sizes": odd(4)}, {"out3": odd(4)}):
        assert _finish(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    assert _round(lib, changed=odd(4), wb=0) == E_WORKSPACE
    assert _finish(lib, labels=odd(8), dense=odd(4), sizes=odd(8), out3=odd(8), wb=0) == E_WORKSPACE


def test_limits_agree_with_graph_csr_and_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import communities
    from rag_arc_amd.encapsulation.database.graph_db import components as C

    lim = C.limits()
    lv = communities.bucket_limits()
    assert lim == {"group": lv["group"], "wave": lv["wave"], "lds": lv["lds"], "round_slack": C.ROUND_SLACK}
    assert (lim["group"], lim["wave"], lim["lds"], lim["round_slack"]) == (8, 64, 8192, 2)        # csrc/graph_csr.h
    assert B.load_library().rarc_components_limits(None) == E_INVALID
    assert [C.round_bound(n) for n in (2, 3, 4, 5, 4096, 4097, (1 << 31) - 2)] == [3, 4, 4, 5, 14, 15, 33]


def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import connected_components, deduplicate_entities, entity_clusters

    for pairs in ([(0, 3)], [(-1, 0)], [(1, 1)], [(0.5, 1)], [(0, 1, 2)], [0, 1, 2]):      # outside [0, n), a loop, no integer, no pairs
        with pytest.raises(ValueError):
            connected_components(3, pairs)
    with pytest.raises(ValueError, match="negative"):
        connected_components(-1, [])
    x = np.eye(4, dtype=np.float32)
    for call in (entity_clusters, deduplicate_entities):
        with pytest.raises(ValueError, match="method.*'wcc'"):
            call(x, method="wcc")
        with pytest.raises(ValueError, match="method"):
            call(x, threshold=7.0, max_iterations=0, method=None)                            # the method is looked at first
    with pytest.raises(ValueError, match="max_iterations"):                                  # the other checks are what they were
        entity_clusters(x, max_iterations=0, method="components")
    with pytest.raises(ValueError, match="threshold"):
        entity_clusters(x, threshold=0.0, method="components")
    with pytest.raises(ValueError, match="min_size"):
        entity_clusters(x, min_size=0, method="components")


def test_an_edgeless_graph_is_answered_on_the_host():
    from rag_arc_amd.encapsulation.database.graph_db import Components, connected_components

    for pairs in ([], np.zeros((0, 2), np.int64)):
        got = connected_components(5, pairs)
        assert isinstance(got, Components) and got.rounds == 0 and got.n_components == 5 and got.largest == (0, 1)
        assert got.labels.dtype == np.int64 and got.labels.tolist() == [0, 1, 2, 3, 4]
        assert got.dense.dtype == np.int32 and got.dense.tolist() == [0, 1, 2, 3, 4]
        assert got.sizes.dtype == np.int64 and got.sizes.tolist() == [1] * 5
    assert connected_components(1, []).n_components == 1 and connected_components(0, []).largest == (-1, 0)


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import connected_components, entity_clusters

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: tests/test_gpu_components.py covers the call")
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        connected_components(4, [(2, 1), (3, 1)])
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        entity_clusters(np.eye(4, dtype=np.float32), method="components")
