"""The passage-projection exports (rarc_ppr_chunks / _scores / _topk, their workspace size and limits) validate their arguments
through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a box without a GPU (the
pointers below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes

import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
BIG = 1 << 60
N, M, NQ, NC, NNZ = 1000, 5000, 8, 700, 3000


def _project(lib, n=N, m=M, nq=NQ, cur=0, ws=P, wb=BIG, row_ptr=P, ent=P, w=P, nc=NC, nnz=NNZ, split=P, n_split=3, cws=P, cb=BIG):
    return lib.rarc_ppr_chunks(n, m, nq, cur, ws, wb, row_ptr, ent, w, nc, nnz, split, n_split, cws, cb, None)


def _scores(lib, nc=NC, nq=NQ, cws=P, cb=BIG, out=P):
    return lib.rarc_ppr_chunks_scores(nc, nq, cws, cb, out, None)


def _topk(lib, nc=NC, nq=NQ, k=10, cws=P, cb=BIG, ids=P, sc=P, cnt=P):
    return lib.rarc_ppr_chunks_topk(nc, nq, k, cws, cb, ids, sc, cnt, None)


CALLS = {"rarc_ppr_chunks": _project, "rarc_ppr_chunks_scores": _scores, "rarc_ppr_chunks_topk": _topk}


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in ("rarc_ppr_chunks_workspace_bytes", "rarc_ppr_chunks", "rarc_ppr_chunks_scores", "rarc_ppr_chunks_topk",
                 "rarc_ppr_chunks_limits"):
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("call,null", [("rarc_ppr_chunks", "ws"), ("rarc_ppr_chunks", "row_ptr"), ("rarc_ppr_chunks", "ent"),
                                       ("rarc_ppr_chunks", "w"), ("rarc_ppr_chunks", "split"), ("rarc_ppr_chunks", "cws"),
                                       ("rarc_ppr_chunks_scores", "cws"), ("rarc_ppr_chunks_scores", "out"),
                                       ("rarc_ppr_chunks_topk", "cws"), ("rarc_ppr_chunks_topk", "ids"), ("rarc_ppr_chunks_topk", "sc"),
                                       ("rarc_ppr_chunks_topk", "cnt")])
def test_null_pointers(call, null):
    lib = B.load_library()
    assert CALLS[call](lib, **{null: None}) == E_INVALID and b"null pointer" in lib.rarc_last_error()
    assert call.encode() + b":" in lib.rarc_last_error()


def test_the_split_list_may_be_null_only_when_it_is_empty():
    lib = B.load_library()
    assert _project(lib, split=None, n_split=0, cb=0) == E_WORKSPACE            # accepted up to the workspace check
    assert _project(lib, split=None, n_split=1) == E_INVALID
    for n_split in (-1, NC + 1):
        assert _project(lib, n_split=n_split) == E_INVALID and b"split chunks" in lib.rarc_last_error()
    assert _project(lib, n_split=NC, cb=0) == E_WORKSPACE


@pytest.mark.parametrize("call", list(CALLS))
@pytest.mark.parametrize("kw", [{"nq": 0}, {"nq": -1}, {"nq": 257}, {"nc": 0}, {"nc": -1}, {"nc": (1 << 31) - 1}])
def test_shapes_out_of_range(call, kw):
    lib = B.load_library()
    rc = CALLS[call](lib, **kw)
    if call == "rarc_ppr_chunks_topk" and kw.get("nc") == (1 << 31) - 1:
        assert rc == E_UNSUPPORTED
    else:
        assert rc == E_INVALID and b"out of range" in lib.rarc_last_error(), lib.rarc_last_error()
    assert lib.rarc_ppr_chunks_workspace_bytes(kw.get("nc", NC), kw.get("nq", NQ)) == 0


@pytest.mark.parametrize("kw", [{"n": 1}, {"n": (1 << 31) - 1}, {"m": 0}, {"m": 1 << 30}, {"nnz": 0}, {"nnz": -5}, {"cur": 2}, {"cur": -1}])
def test_the_projection_refuses_the_graph_shapes_the_mentions_and_the_slot(kw):
    lib = B.load_library()
    assert _project(lib, **kw) == E_INVALID
    assert (b"slot" if "cur" in kw else b"out of range") in lib.rarc_last_error()


def test_top_k_out_of_range():
    lib = B.load_library()
    for k in (0, -1, 8193):
        assert _topk(lib, k=k) == E_INVALID and b"top_k" in lib.rarc_last_error()
    assert _topk(lib, k=1, cb=0) == E_WORKSPACE and _topk(lib, k=8192, cb=0) == E_WORKSPACE


def test_the_limits_themselves_are_accepted():
    lib = B.load_library()
    for nc, nq in ((1, 1), ((1 << 31) - 2, 256), (NC, 256)):
        assert lib.rarc_ppr_chunks_workspace_bytes(nc, nq) > 0
        assert _project(lib, nc=nc, nq=nq, nnz=1, n_split=0, cb=0) == E_WORKSPACE and _scores(lib, nc=nc, nq=nq, cb=0) == E_WORKSPACE
    assert _project(lib, cur=1, cb=0) == E_WORKSPACE


def test_topk_refuses_2_to_the_24_chunks_and_names_the_limit_but_the_scores_do_not():
    """the argument check and a workspace-bytes query suffice: nothing that large is allocated"""
    lib = B.load_library()
    assert lib.rarc_ppr_chunks_workspace_bytes(1 << 24, 1) >= 2 * 8 * (1 << 24)
    assert _topk(lib, nc=1 << 24, nq=1) == E_UNSUPPORTED
    assert b"2^24" in lib.rarc_last_error() and b"16777216" in lib.rarc_last_error()
    assert _topk(lib, nc=(1 << 24) - 1, nq=1, cb=0) == E_WORKSPACE
    assert _scores(lib, nc=1 << 24, nq=1, cb=0) == E_WORKSPACE
    assert _project(lib, nc=1 << 24, nq=1, cb=0) == E_WORKSPACE


def test_short_workspaces():
    lib = B.load_library()
    need, pneed = lib.rarc_ppr_chunks_workspace_bytes(NC, NQ), lib.rarc_ppr_workspace_bytes(N, M, NQ)
    assert need >= 2 * NC * NQ * 8                # S and the keys
    assert lib.rarc_ppr_chunks_workspace_bytes(NC, 2 * NQ) > need and lib.rarc_ppr_chunks_workspace_bytes(2 * NC, NQ) > need
    for name, call in CALLS.items():
        assert call(lib, cb=need - 1) == E_WORKSPACE and b"chunk workspace" in lib.rarc_last_error()
    assert _project(lib, cb=need, wb=pneed - 1) == E_WORKSPACE and b"workspace" in lib.rarc_last_error()
    assert b"chunk workspace" not in lib.rarc_last_error()


def test_misaligned_pointers():
    lib = B.load_library()
    odd = lambda a: ctypes.c_void_p(4096 + a)     # noqa: E731
    for call in CALLS.values():
        assert call(lib, cws=odd(128)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    assert _project(lib, ws=odd(8)) == E_INVALID and b"256-byte aligned" in lib.rarc_last_error()
    for kw in ({"row_ptr": odd(4)}, {"ent": odd(2)}, {"w": odd(1)}, {"split": odd(2)}):
        assert _project(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()
    assert _project(lib, row_ptr=odd(8), ent=odd(4), w=odd(4), split=odd(4), cb=0) == E_WORKSPACE
    assert _scores(lib, out=odd(4)) == E_INVALID and b"8-byte aligned" in lib.rarc_last_error()
    assert _scores(lib, out=odd(8), cb=0) == E_WORKSPACE and _topk(lib, ids=odd(8), sc=odd(8), cnt=odd(4), cb=0) == E_WORKSPACE
    for kw in ({"ids": odd(4)}, {"sc": odd(4)}, {"cnt": odd(2)}):
        assert _topk(lib, **kw) == E_INVALID and b"aligned to its element" in lib.rarc_last_error()


def test_limits():
    from rag_arc_amd.encapsulation.database.graph_db import pagerank, passages

    lim = passages.limits()
    assert lim["split_degree"] == pagerank.limits()["split_degree"] == 64
    assert 1 << lim["weight_bits"] == passages.MAX_MENTION_WEIGHT == 4096
    assert lim["score_shift"] == passages.SCORE_SHIFT == 40 - lim["weight_bits"]
    assert 1 << lim["topk_chunk_bits"] == passages.MAX_TOPK_CHUNKS
    assert B.load_library().rarc_ppr_chunks_limits(None) == E_INVALID
    out = (ctypes.c_int * 6)()
    B.load_library().rarc_ppr_limits(out)
    assert list(out) == [64, 32, 256, 64, 8192, 24]              # the six words of rarc_ppr_limits are what they were


def test_the_host_csr_merges_sorts_and_lists_the_split_chunks():
    import numpy as np

    from rag_arc_amd.encapsulation.database.graph_db.passages import mention_csr

    row_ptr, ent, w, split = mention_csr(4, 5, [(2, 3), (0, 1), (2, 0), (0, 1), (3, 4)], [2, 1, 4, 3, 4095])
    assert row_ptr.tolist() == [0, 1, 1, 3, 4] and ent.tolist() == [1, 0, 3, 4] and w.tolist() == [4, 4, 2, 4095]
    assert (row_ptr.dtype, ent.dtype, w.dtype, split.dtype) == (np.int64, np.int32, np.uint32, np.int32) and split.size == 0
    big = [(1, e) for e in range(65)] + [(0, e) for e in range(64)]
    assert mention_csr(3, 70, big, split_degree=64)[3].tolist() == [1]
    assert mention_csr(2, 3, [(0, 1)])[2].tolist() == [1]                         # unit weights by default


def test_mention_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    for nc, n, mentions in ((3, 4, [(3, 0)]), (3, 4, [(-1, 0)]), (3, 4, [(0, 4)]), (3, 4, [(0, -1)]), (3, 4, [(0, 1, 2)]), (3, 4, []),
                            (0, 4, [(0, 0)]), (3, 4, [(0.5, 1)])):
        with pytest.raises(ValueError):
            MentionMap(nc, n, mentions)
    for w in ([0], [1.5], [1, 2], [-3]):
        with pytest.raises(ValueError):
            MentionMap(3, 4, [(0, 1)], weights=w)
    with pytest.raises(B.RarcUnsupported, match="2\\^12"):
        MentionMap(3, 4, [(0, 1)], weights=[4096])
    with pytest.raises(B.RarcUnsupported, match="add up to 4096.*2\\^12"):
        MentionMap(3, 4, [(0, 1), (2, 2), (0, 1)], weights=[4000, 7, 96])
    with pytest.raises(B.RarcUnsupported, match="2\\^31"):
        MentionMap((1 << 31) - 1, 4, [(0, 1)])


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    if torch.cuda.is_available():
        assert MentionMap(3, 4, [(0, 1), (2, 3)], weights=[4095, 1]).nnz == 2
        return
    with pytest.raises(B.RarcError, match="no CPU fallback"):
        MentionMap(3, 4, [(0, 1), (2, 3)], weights=[4095, 1])
