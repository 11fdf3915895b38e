"""The k-hop exports (rarc_khop_seed / _step / _counts / _levels / _list / _chunks, their workspace size and limits) validate
their arguments through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a
GPU (the pointers below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
BIG = 1 << 60
N, M, NQ, HOPS, NC, NNZ = 1000, 5000, 8, 3, 700, 3000
DECAY = (ctypes.c_uint32 * 9)(4096, 1024, 256, 64, 16, 4, 1, 0, 0)


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _seed(lib, n=N, m=M, seeds=P, nq=NQ, s=5, hops=HOPS, ws=P, wb=BIG):
    return lib.rarc_khop_seed(n, m, seeds, nq, s, hops, ws, wb, None)


def _step(lib, graph=P, gb=BIG, n=N, m=M, nq=NQ, hops=HOPS, hop=1, ws=P, wb=BIG, grew=P):
    return lib.rarc_khop_step(graph, gb, n, m, nq, hops, hop, ws, wb, grew, None)


def _counts(lib, n=N, m=M, nq=NQ, hops=HOPS, ws=P, wb=BIG, out=P):
    return lib.rarc_khop_counts(n, m, nq, hops, ws, wb, out, None)


def _levels(lib, n=N, m=M, nq=NQ, hops=HOPS, ws=P, wb=BIG, out=P):
    return lib.rarc_khop_levels(n, m, nq, hops, ws, wb, out, None)


def _list(lib, n=N, m=M, nq=NQ, hops=HOPS, mv=100, ws=P, wb=BIG, ids=P, hp=P, cnt=P):
    return lib.rarc_khop_list(n, m, nq, hops, mv, ws, wb, ids, hp, cnt, None)


def _chunks(lib, n=N, m=M, nq=NQ, hops=HOPS, decay=DECAY, ws=P, wb=BIG, row_ptr=P, ent=P, w=P, nc=NC, nnz=NNZ, split=P, n_split=3, cws=P,
            cb=BIG):
    decay = ctypes.cast(decay, ctypes.c_void_p) if decay is not None else None
    return lib.rarc_khop_chunks(n, m, nq, hops, decay, ws, wb, row_ptr, ent, w, nc, nnz, split, n_split, cws, cb, None)


CALLS = {"rarc_khop_seed": _seed, "rarc_khop_step": _step, "rarc_khop_counts": _counts, "rarc_khop_levels": _levels, "rarc_khop_list": _list,
         "rarc_khop_chunks": _chunks}


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in list(CALLS) + ["rarc_khop_workspace_bytes", "rarc_khop_limits"]:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("call,null", [("rarc_khop_seed", "seeds"), ("rarc_khop_seed", "ws"), ("rarc_khop_step", "graph"), ("rarc_khop_step", "ws"),
                                       ("rarc_khop_counts", "ws"), ("rarc_khop_counts", "out"), ("rarc_khop_levels", "ws"),
                                       ("rarc_khop_levels", "out"), ("rarc_khop_list", "ws"), ("rarc_khop_list", "ids"), ("rarc_khop_list", "hp"),
                                       ("rarc_khop_list", "cnt"), ("rarc_khop_chunks", "decay"), ("rarc_khop_chunks", "ws"),
                                       ("rarc_khop_chunks", "row_ptr"), ("rarc_khop_chunks", "ent"), ("rarc_khop_chunks", "w"),
                                       ("rarc_khop_chunks", "split"), ("rarc_khop_chunks", "cws")])
def test_null_pointers(call, null):
    lib = B.load_library()
    assert CALLS[call](lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()


def test_the_grew_word_and_an_empty_split_list_may_be_null():
    lib = B.load_library()
    assert _step(lib, grew=None, wb=0) == E_WORKSPACE                       # accepted up to the workspace check
    assert _chunks(lib, split=None, n_split=0, cb=0) == E_WORKSPACE
    assert _chunks(lib, split=None, n_split=1) == E_INVALID
    for n_split in (-1, NC + 1):
        assert _chunks(lib, n_split=n_split) == E_INVALID and b"split chunks" in lib.rarc_last_error()


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nq": 0}, {"nq": -1}, {"nq": 257}, {"hops": -1}])
def test_shapes_out_of_range(call, kw):
    lib = B.load_library()
    assert CALLS[call](lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()
    assert lib.rarc_khop_workspace_bytes(kw.get("n", N), kw.get("m", M), kw.get("nq", NQ), kw.get("hops", HOPS)) == 0


@pytest.mark.parametrize("call", list(CALLS))
def test_more_than_8_hops_is_unsupported_and_names_the_limit(call):
    lib = B.load_library()
    assert CALLS[call](lib, hops=9) == E_UNSUPPORTED and b"hops=9" in lib.rarc_last_error() and b"8" in lib.rarc_last_error()
    assert lib.rarc_khop_workspace_bytes(N, M, NQ, 9) == 0 and lib.rarc_khop_workspace_bytes(N, M, NQ, 8) > 0


def test_seed_slots_the_hop_the_list_length_the_mentions_and_the_decay():
    lib = B.load_library()
    for s in (0, -1, 65):
        assert _seed(lib, s=s) == E_INVALID and b"seed slots" in lib.rarc_last_error()
    assert _seed(lib, s=1, wb=0) == E_WORKSPACE and _seed(lib, s=64, wb=0) == E_WORKSPACE
    for hop in (0, -1, HOPS + 1):
        assert _step(lib, hop=hop) == E_INVALID and b"hop " in lib.rarc_last_error()
    assert _step(lib, hops=0, hop=1) == E_INVALID                           # nothing to step at hops = 0
    assert _step(lib, hop=HOPS, wb=0) == E_WORKSPACE
    for mv in (0, -1):
        assert _list(lib, mv=mv) == E_INVALID and b"max_vertices" in lib.rarc_last_error()
    assert _list(lib, mv=65537) == E_UNSUPPORTED and b"65536" in lib.rarc_last_error()
    assert _list(lib, mv=65536, wb=0) == E_WORKSPACE and _list(lib, mv=1, wb=0) == E_WORKSPACE
    for kw in ({"nc": 0}, {"nc": -1}, {"nc": (1 << 31) - 1}, {"nnz": 0}, {"nnz": -5}):
        assert _chunks(lib, **kw) == E_INVALID and b"out of range" in lib.rarc_last_error()
    bad = (ctypes.c_uint32 * 9)(4096, 65537, 0, 0, 0, 0, 0, 0, 0)
    assert _chunks(lib, decay=bad) == E_INVALID and b"decay[1]=65537" in lib.rarc_last_error() and b"2^16" in lib.rarc_last_error()
    assert _chunks(lib, decay=bad, hops=0, cb=0) == E_WORKSPACE              # only hops + 1 entries are read
    top = (ctypes.c_uint32 * 9)(*([65536] * 9))
    assert _chunks(lib, decay=top, hops=8, cb=0) == E_WORKSPACE


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for n, m, nq, hops in ((2, 1, 1, 0), ((1 << 31) - 2, (1 << 30) - 1, 256, 8), (N, M, 256, 8), (N, M, 64, 0)):
        assert lib.rarc_khop_workspace_bytes(n, m, nq, hops) > 0
        for name, call in CALLS.items():
            kw = {"hop": max(hops, 1)} if name == "rarc_khop_step" else {}
            if name == "rarc_khop_step" and hops == 0:
                continue
            assert call(lib, n=n, m=m, nq=nq, hops=hops, wb=0, **kw) == E_WORKSPACE, name


def test_short_workspaces():
    lib = B.load_library()
    need = lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS)
    assert need >= (HOPS + 2) * N * 8                                        # seen and the levels, one word per vertex up to 64 queries
    assert lib.rarc_khop_workspace_bytes(N, M, 64, HOPS) == need < lib.rarc_khop_workspace_bytes(N, M, 65, HOPS)
    assert lib.rarc_khop_workspace_bytes(N, M, NQ, HOPS + 1) > need and lib.rarc_khop_workspace_bytes(2 * N, M, NQ, HOPS) > need
    for name, call in CALLS.items():
        assert call(lib, wb=need - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error(), name
    assert _step(lib, wb=need, gb=lib.rarc_graph_csr_workspace_bytes(N, M) - 1) == E_WORKSPACE and b"graph workspace" in lib.rarc_last_error()
    cneed = lib.rarc_ppr_chunks_workspace_bytes(NC, NQ)
    assert _chunks(lib, wb=need, cb=cneed - 1) == E_WORKSPACE and b"chunk workspace" in lib.rarc_last_error()


def test_misaligned_pointers():
    lib = B.load_library()
    for name, call in CALLS.items():
        assert call(lib, ws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error(), name
    assert _chunks(lib, cws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _step(lib, graph=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _seed(lib, seeds=odd(4)) == E_INVALID and b"8-byte aligned" in lib.rarc_last_error()
    assert _step(lib, grew=odd(2)) == E_INVALID and b"4-byte aligned" in lib.rarc_last_error()
    assert _counts(lib, out=odd(2)) == E_INVALID and b"4-byte aligned" in lib.rarc_last_error()
    for kw in ({"ids": odd(4)}, {"hp": odd(2)}, {"cnt": odd(2)}):
        assert _list(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    for kw in ({"row_ptr": odd(4)}, {"ent": odd(2)}, {"w": odd(1)}, {"split": odd(2)}):
        assert _chunks(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    assert _seed(lib, seeds=odd(8), wb=0) == E_WORKSPACE and _step(lib, grew=odd(4), wb=0) == E_WORKSPACE
    assert _levels(lib, out=odd(1), wb=0) == E_WORKSPACE                     # bytes: any address
    assert _list(lib, ids=odd(8), hp=odd(4), cnt=odd(4), wb=0) == E_WORKSPACE
    assert _chunks(lib, row_ptr=odd(8), ent=odd(4), w=odd(4), split=odd(4), cb=0) == E_WORKSPACE


def test_limits_agree_with_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K
    from rag_arc_amd.encapsulation.database.graph_db import pagerank

    lim = K.limits()
    assert lim == {"max_hops": K.MAX_HOPS, "max_batch": K.MAX_BATCH, "max_seeds": K.MAX_SEEDS, "max_vertices": K.MAX_LIST_VERTICES,
                   "split_degree": pagerank.limits()["split_degree"]}
    assert (K.MAX_HOPS, K.MAX_BATCH, K.MAX_SEEDS, K.MAX_LIST_VERTICES) == (8, 256, 64, 65536)
    assert B.load_library().rarc_khop_limits(None) == E_INVALID
    assert K.default_decay(2).tolist() == [4096, 1024, 256] and K.default_decay(8).max() <= K.MAX_DECAY


def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import k_hop
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as K

    pairs = [(0, 1), (1, 2)]
    for seeds in ([[3]], [[-2]], [[0.5]], [list(range(3)) * 22], []):        # outside [0, n), no integer, 66 seeds, no queries
        with pytest.raises(ValueError):
            k_hop(3, pairs, seeds)
    with pytest.raises(ValueError, match="hops"):
        k_hop(3, pairs, [[0]], hops=-1)
    with pytest.raises(B.RarcUnsupported, match="hops=9.*8"):
        k_hop(3, pairs, [[0]], hops=9)
    with pytest.raises(B.RarcUnsupported, match="65536"):
        k_hop(3, pairs, [[0]], max_vertices=65537)
    with pytest.raises(ValueError, match="max_vertices"):
        k_hop(3, pairs, [[0]], max_vertices=0)
    assert K.host_seeds(5, [[4, 4], [], [0]]).tolist() == [[4, 4], [-1, -1], [0, -1]]
    for decay, hops in (([4096, 1024], 2), ([1, 2, 65537], 2), ([1, -1, 0], 2), ([1.5, 1, 1], 2)):
        with pytest.raises(ValueError, match="decay"):
            K.check_decay(decay, hops)
    assert K.check_decay([65536, 0, 7], 2).tolist() == [65536, 0, 7] and K.check_decay(None, 1).tolist() == [4096, 1024]


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import k_hop

    if torch.cuda.is_available():
        assert k_hop(3, [(0, 1), (1, 2)], [[0]], hops=1).tolist() == [[0, 1, 255]]
        return
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        k_hop(3, [(0, 1), (1, 2)], [[0]], hops=1)


def test_an_unknown_expansion_is_refused_before_anything_is_built():
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    with pytest.raises(ValueError, match="expansion"):
        HipGraphRetriever(None, None, None, None, [], expansion="bfs")
