"""The co-occurrence exports (rarc_cooccur_count / _emit / _edges, their workspace sizes and limits) validate their arguments
through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a GPU (the pointers
below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 60
NC, NNZ, N = 1000, 5000, 700


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _count(lib, row_ptr=P, ent=P, w=P, n_chunks=NC, nnz=NNZ, n=N, max_mentions=64, ws=P, wb=BIG, out4=P):
    return lib.rarc_cooccur_count(row_ptr, ent, w, n_chunks, nnz, n, max_mentions, ws, wb, out4, None)


def _emit(lib, row_ptr=P, ent=P, w=P, n_chunks=NC, nnz=NNZ, n=N, mode=1, ws=P, wb=BIG, keys=P, values=P, total=100):
    return lib.rarc_cooccur_emit(row_ptr, ent, w, n_chunks, nnz, n, mode, ws, wb, keys, values, total, None)


def _edges(lib, keys=P, sums=P, distinct=100, n=N, min_weight=1, ws=P, wb=BIG, pairs=P, weights=P, out3=P):
    return lib.rarc_cooccur_edges(keys, sums, distinct, n, min_weight, ws, wb, pairs, weights, out3, None)


CALLS = {"rarc_cooccur_count": _count, "rarc_cooccur_emit": _emit, "rarc_cooccur_edges": _edges}
CSR_CALLS = {k: CALLS[k] for k in ("rarc_cooccur_count", "rarc_cooccur_emit")}


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in list(CALLS) + ["rarc_cooccur_workspace_bytes", "rarc_cooccur_edges_workspace_bytes", "rarc_cooccur_limits"]:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("call,null", [("rarc_cooccur_count", k) for k in ("row_ptr", "ent", "w", "ws", "out4")]
                         + [("rarc_cooccur_emit", k) for k in ("row_ptr", "ent", "w", "ws", "keys", "values")]
                         + [("rarc_cooccur_edges", k) for k in ("keys", "sums", "ws", "pairs", "weights", "out3")])
def test_null_pointers(call, null):
    lib = B.load_library()
    assert CALLS[call](lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()


def test_the_values_may_be_null_in_mode_count():
    lib = B.load_library()
    assert _emit(lib, mode=0, values=None, wb=0) == E_WORKSPACE                    # accepted up to the workspace check


@pytest.mark.parametrize("call", list(CSR_CALLS))
@pytest.mark.parametrize("kw", [{"n_chunks": 0}, {"n_chunks": -1}, {"n_chunks": (1 << 31) - 1}, {"nnz": 0}, {"nnz": -5}, {"nnz": 1 << 31},
                                {"n": 1}, {"n": 0}, {"n": -3}, {"n": (1 << 31) - 1}])
def test_shapes_out_of_range(call, kw):
    lib = B.load_library()
    assert CALLS[call](lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()
    if "n" not in kw:
        assert lib.rarc_cooccur_workspace_bytes(kw.get("n_chunks", NC), kw.get("nnz", NNZ)) == 0


@pytest.mark.parametrize("kw", [{"distinct": 0}, {"distinct": -1}, {"distinct": 1 << 31}, {"n": 1}, {"n": (1 << 31) - 1}, {"min_weight": 0},
                                {"min_weight": -2}])
def test_edges_arguments_out_of_range(kw):
    lib = B.load_library()
    assert _edges(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert b"rarc_cooccur_edges:" in lib.rarc_last_error()
    if "distinct" in kw:
        assert lib.rarc_cooccur_edges_workspace_bytes(kw["distinct"]) == 0


def test_max_mentions_mode_and_total_out_of_range():
    lib = B.load_library()
    lim = (ctypes.c_int * 4)()
    assert lib.rarc_cooccur_limits(lim) == 0
    for mm in (1, 0, -1, lim[1] + 1):
        assert _count(lib, max_mentions=mm) == E_INVALID and b"rarc_cooccur_count: max_mentions" in lib.rarc_last_error()
    for mm in (2, lim[1]):
        assert _count(lib, max_mentions=mm, wb=0) == E_WORKSPACE
    for mode in (-1, 2, 7):
        assert _emit(lib, mode=mode) == E_INVALID and b"rarc_cooccur_emit: mode" in lib.rarc_last_error()
    for total in (0, -1, 1 << lim[3]):
        assert _emit(lib, total=total) == E_INVALID and b"rarc_cooccur_emit: T=" in lib.rarc_last_error()
    assert _emit(lib, total=(1 << lim[3]) - 1, wb=0) == E_WORKSPACE


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for nc, nnz, n in ((1, 1, 2), ((1 << 31) - 2, (1 << 31) - 1, (1 << 31) - 2), (NC, NNZ, N)):
        assert lib.rarc_cooccur_workspace_bytes(nc, nnz) > 0
        for name, call in CSR_CALLS.items():
            assert call(lib, n_chunks=nc, nnz=nnz, n=n, wb=0) == E_WORKSPACE, name
    for distinct, n in ((1, 2), ((1 << 31) - 1, (1 << 31) - 2)):
        assert lib.rarc_cooccur_edges_workspace_bytes(distinct) > 0
        assert _edges(lib, distinct=distinct, n=n, min_weight=1 << 40, wb=0) == E_WORKSPACE


def test_short_workspaces():
    lib = B.load_library()
    need = lib.rarc_cooccur_workspace_bytes(NC, NNZ)
    assert need >= NC * (4 + 8 + 4 + 4)                                      # the counts, the offsets and the two lists
    assert lib.rarc_cooccur_workspace_bytes(NC, 1) == need                   # the state is per chunk
    assert lib.rarc_cooccur_workspace_bytes(2 * NC, NNZ) > need
    for name, call in CSR_CALLS.items():
        assert call(lib, wb=need - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error(), name
        assert name.encode() + b":" in lib.rarc_last_error()
    eneed = lib.rarc_cooccur_edges_workspace_bytes(100)
    assert 0 < eneed < lib.rarc_cooccur_edges_workspace_bytes(1 << 20)
    assert _edges(lib, wb=eneed - 1) == E_WORKSPACE and b"rarc_cooccur_edges: workspace" in lib.rarc_last_error()


def test_misaligned_pointers():
    lib = B.load_library()
    for name, call in CALLS.items():
        assert call(lib, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error(), name
        assert name.encode() + b":" in lib.rarc_last_error()
    for name, call in CSR_CALLS.items():
        for kw in ({"row_ptr": odd(4)}, {"ent": odd(2)}, {"w": odd(2)}):
            assert call(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), (name, kw)
        assert call(lib, row_ptr=odd(8), ent=odd(4), w=odd(4), wb=0) == E_WORKSPACE
    assert _count(lib, out4=odd(4)) == E_INVALID and b"8-byte aligned" in lib.rarc_last_error()
    for kw in ({"keys": odd(4)}, {"values": odd(2)}):
        assert _emit(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    for kw in ({"keys": odd(4)}, {"sums": odd(4)}, {"pairs": odd(4)}, {"weights": odd(2)}, {"out3": odd(4)}):
        assert _edges(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    assert _edges(lib, keys=odd(8), sums=odd(8), pairs=odd(8), weights=odd(4), out3=odd(8), wb=0) == E_WORKSPACE


def test_limits_agree_with_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence as C
    from rag_arc_amd.encapsulation.database.graph_db import merge, passages

    lim = C.limits()
    assert lim == {"wave_degree": 64, "max_mentions": C.MAX_MAX_MENTIONS, "product_bits": 24, "max_total_pairs": merge.MAX_COUNT}
    assert 1 << lim["product_bits"] == passages.MAX_MENTION_WEIGHT ** 2 and lim["max_mentions"] == 4096
    assert B.load_library().rarc_cooccur_limits(None) == E_INVALID


class _Map:
    """what the argument checks look at before any device is needed"""
    n_entities = 10


def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.core.retrieval.graph import HipGraphRetriever
    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence as C
    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence_graph, cooccurrence_pairs

    with pytest.raises(ValueError, match="MentionMap"):
        cooccurrence_pairs([(0, 1)])
    for kw, what in (({"weight": "jaccard"}, "weight"), ({"weight": None}, "weight"), ({"min_weight": 0}, "min_weight"),
                     ({"min_weight": 1.5}, "min_weight"), ({"max_mentions": 1}, "max_mentions"), ({"max_mentions": 4097}, "max_mentions")):
        args = {"weight": "count", "min_weight": 1, "max_mentions": 64, **kw}
        with pytest.raises(ValueError, match=what):
            C.check_arguments(10, **args)
        with pytest.raises(ValueError, match=what):
            cooccurrence_graph(3, 10, [(0, 1), (0, 2)], **kw)
        with pytest.raises(ValueError, match=what):
            HipGraphRetriever.from_arrays(None, np.eye(10, dtype=np.float32), None, [(0, 1), (0, 2)], ["a", "b", "c"],
                                          **{("cooccurrence_weight" if k == "weight" else k): v for k, v in kw.items()})
    assert C.check_arguments(2, "product", 3, 4096) == (1, 3, 4096) and C.check_arguments(2, "count", 1, 2) == (0, 1, 2)
    with pytest.raises(ValueError, match="at least 2 entities"):
        C.check_arguments(1, "count", 1, 64)
    with pytest.raises(ValueError, match="at least 2 entities"):
        cooccurrence_graph(3, 1, [(0, 0)])
    with pytest.raises(ValueError, match="pair_weights"):
        HipGraphRetriever.from_arrays(None, np.eye(10, dtype=np.float32), None, [(0, 1)], ["a"], pair_weights=[1])
    for mentions in ([(0, 10)], [(3, 0)], [(0.5, 1)]):                                      # MentionMap's own refusals come first
        with pytest.raises(ValueError):
            cooccurrence_graph(3, 10, mentions)


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence_graph

    if torch.cuda.is_available():
        pytest.skip("a GPU is visible: tests/test_gpu_cooccur.py covers the call")
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        cooccurrence_graph(2, 4, [(0, 1), (0, 2), (1, 2), (1, 3)])
