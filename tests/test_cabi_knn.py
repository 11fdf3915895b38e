"""rarc_knn_graph / rarc_knn_graph_workspace_bytes validate their arguments through the C-ABI before anything touches a device:
error codes with a rarc_last_error text on a box without a GPU (the pointers below are never dereferenced)."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3


def _call(lib, rows=P, ld=768, n=1000, d=768, top_k=10, cutoff=0.85, ws=P, ws_bytes=1 << 40, cap=256, ids=P, cos=P, cnt=P, flags=P):
    return lib.rarc_knn_graph(rows, ld, n, d, top_k, ctypes.c_double(cutoff), ws, ws_bytes, cap, ids, cos, cnt, flags, None)


@pytest.mark.parametrize("null", ["rows", "ws", "ids", "cos", "cnt", "flags"])
def test_null_pointers(null):
    lib = B.load_library()
    assert _call(lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()


@pytest.mark.parametrize("kw,text", [({"top_k": 0}, b"top_k"), ({"top_k": 257}, b"top_k"), ({"cutoff": 1.5}, b"cutoff"),
                                     ({"cutoff": float("nan")}, b"cutoff"), ({"cutoff": -1.0000001}, b"cutoff"),
                                     ({"d": 0}, b"bad shape"), ({"d": 4097, "ld": 4097}, b"bad shape"), ({"ld": 767}, b"bad shape"),
                                     ({"n": -1}, b"bad shape"), ({"n": 0x7fffff00}, b"bad shape"), ({"cap": 0}, b"bad shape")])
def test_bad_arguments(kw, text):
    lib = B.load_library()
    assert _call(lib, **kw) == E_INVALID
    assert text in lib.rarc_last_error(), lib.rarc_last_error()


def test_short_workspace():
    lib = B.load_library()
    need = lib.rarc_knn_graph_workspace_bytes(1000, 768, 10, 256)
    # the fp16 image of 1024 padded rows, their float64 inverse norms, 4096 lists of 256 entries
    assert need >= 1024 * 768 * 2 + 1024 * 8 + 4096 * 256 * 8
    assert _call(lib, ws_bytes=need - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error()
    assert _call(lib, ws_bytes=0) == E_WORKSPACE
    assert lib.rarc_knn_graph_workspace_bytes(1000, 768, 10, 1024) > need            # grows with the lists


@pytest.mark.parametrize("args", [(0, 768, 10, 256), (-5, 768, 10, 256), (0x7fffff00, 768, 10, 256), (1000, 0, 10, 256),
                                  (1000, 4097, 10, 256), (1000, 768, 0, 256), (1000, 768, 257, 256), (1000, 768, 10, 0)])
def test_workspace_bytes_is_zero_on_bad_arguments(args):
    assert B.load_library().rarc_knn_graph_workspace_bytes(*args) == 0


def test_the_limits_themselves_are_accepted():
    """top_k 1 and 256, cutoff -1 and 1, d 1 and 4096 pass validation: with a workspace one byte short the call gets as far as
    the workspace check (and no further: nothing is launched)."""
    lib = B.load_library()
    for kw in ({"top_k": 1}, {"top_k": 256}, {"cutoff": -1.0}, {"cutoff": 1.0}, {"d": 1, "ld": 1}, {"d": 4096, "ld": 4096}):
        d, k = kw.get("d", 768), kw.get("top_k", 10)
        need = lib.rarc_knn_graph_workspace_bytes(1000, d, k, 256)
        assert need > 0 and _call(lib, ws_bytes=need - 1, **kw) == E_WORKSPACE, kw


def test_python_surface_refuses_before_it_needs_a_device():
    from rag_arc_amd.encapsulation.database.graph_db import knn_graph

    x = [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]]
    for kw in ({"top_k": 0}, {"similarity_cutoff": 1.5}, {"similarity_cutoff": -1.5}, {"similarity_cutoff": float("nan")},
               {"similarity_cutoff": float("inf")}):
        with pytest.raises(ValueError):
            knn_graph(x, **kw)
    with pytest.raises(B.RarcUnsupported, match="256"):
        knn_graph(x, top_k=257)


def test_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rag_arc_amd.encapsulation.database.graph_db import knn_graph

    with pytest.raises(B.RarcError, match="no CPU fallback"):
        knn_graph([[1.0, 0.0], [0.0, 1.0]])
