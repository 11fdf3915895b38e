"""The entity-merging exports (rarc_sort_reduce, rarc_merge_plan / _pairs / _mentions / _relations, their workspace sizes and
limits) validate their arguments through the C-ABI before anything touches a device: error codes with a rarc_last_error text on a
box without a GPU (the pointers below are never dereferenced).  The Python surface refuses what it must before it needs a device."""
import ctypes
import types

import numpy as np
import pytest

from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 60
N_LIMIT = (1 << 31) - 1         # n < 2^31 - 1, as the Louvain entries limit it


def odd(a):
    return ctypes.c_void_p(4096 + a)


def _sort(lib, keys=P, vals=P, count=1000, bits=40, ws=P, wb=BIG, ok=P, osum=P, out2=P):
    return lib.rarc_sort_reduce(keys, vals, count, bits, ws, wb, ok, osum, out2, None)


def _plan(lib, labels=P, rich=P, n=1000, ws=P, wb=BIG, primary=P, new_id=P, kept=P, removed=P, cnt=P):
    return lib.rarc_merge_plan(labels, rich, n, ws, wb, primary, new_id, kept, removed, cnt, None)


def _pairs(lib, pairs=P, w=P, m=5000, new_id=P, n=1000, ws=P, wb=BIG, op=P, ow=P, out5=P):
    return lib.rarc_merge_pairs(pairs, w, m, new_id, n, ws, wb, op, ow, out5, None)


def _mentions(lib, row_ptr=P, ent=P, w=P, nc=300, nnz=5000, new_id=P, n=1000, ws=P, wb=BIG, orp=P, oe=P, ow=P, osp=P, out6=P):
    return lib.rarc_merge_mentions(row_ptr, ent, w, nc, nnz, new_id, n, ws, wb, orp, oe, ow, osp, out6, None)


def _relations(lib, rel=P, r=7000, new_id=P, n=1000, ws=P, wb=BIG, orel=P, orows=P, out3=P):
    return lib.rarc_merge_relations(rel, r, new_id, n, ws, wb, orel, orows, out3, None)


ENTRIES = {"rarc_sort_reduce": _sort, "rarc_merge_plan": _plan, "rarc_merge_pairs": _pairs, "rarc_merge_mentions": _mentions,
           "rarc_merge_relations": _relations}
OPTIONAL = {"vals", "rich", "w"}                                       # null = every value 1 / all 0 / unit weights


def _pointer_args(fn):
    import inspect

    return [k for k, v in inspect.signature(fn).parameters.items() if v.default is P]


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in list(ENTRIES) + ["rarc_sort_reduce_workspace_bytes", "rarc_sort_reduce_limits", "rarc_merge_plan_workspace_bytes",
                                 "rarc_merge_pairs_workspace_bytes", "rarc_merge_mentions_workspace_bytes", "rarc_merge_relations_workspace_bytes"]:
        assert name in B.SIGNATURES and getattr(lib, name)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_null_pointers(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    for arg in _pointer_args(fn):
        if arg in OPTIONAL and entry != "rarc_merge_mentions":         # (a CSR always has weights)
            assert fn(lib, **{arg: None}, wb=0) == E_WORKSPACE, (entry, arg)
        else:
            assert fn(lib, **{arg: None}) == E_INVALID and f"{entry}: null pointer".encode() in lib.rarc_last_error(), (entry, arg)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_misaligned_pointers(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    for arg in _pointer_args(fn):
        if arg == "ws":
            assert fn(lib, ws=odd(128)) == E_INVALID and f"{entry}: the workspace is not 256-byte aligned".encode() in lib.rarc_last_error()
        else:
            assert fn(lib, **{arg: odd(2)}) == E_INVALID and b"aligned to its element" in lib.rarc_last_error(), (entry, arg)
            assert entry.encode() in lib.rarc_last_error()
    four = {"vals", "rich", "w", "ow", "ent", "oe", "osp"}
    assert fn(lib, **{a: odd(4 if a in four else 8) for a in _pointer_args(fn) if a != "ws"}, wb=0) == E_WORKSPACE


def test_the_ranges_of_the_sort():
    lib = B.load_library()
    for bits in (0, 63, -1, 64):
        assert _sort(lib, bits=bits) == E_INVALID and b"rarc_sort_reduce: key_bits" in lib.rarc_last_error() and b"62" in lib.rarc_last_error()
    for count in (0, -1, 1 << 31, 1 << 40):
        assert _sort(lib, count=count) == E_INVALID and b"rarc_sort_reduce: count" in lib.rarc_last_error() and b"2^31" in lib.rarc_last_error()
        assert lib.rarc_sort_reduce_workspace_bytes(count) == 0
    for count, bits in ((1, 1), (1, 62), ((1 << 31) - 1, 62)):
        assert lib.rarc_sort_reduce_workspace_bytes(count) > 0 and _sort(lib, count=count, bits=bits, wb=0) == E_WORKSPACE


@pytest.mark.parametrize("entry", ["rarc_merge_plan", "rarc_merge_pairs", "rarc_merge_mentions", "rarc_merge_relations"])
def test_n_is_limited_as_the_louvain_entries_limit_it(entry):
    lib, fn = B.load_library(), ENTRIES[entry]
    for n in (0, -1, N_LIMIT, 1 << 40):
        assert fn(lib, n=n) == E_INVALID and f"{entry}: n={n} out of range".encode() in lib.rarc_last_error()
    for n in (1, 2, N_LIMIT - 1):
        assert fn(lib, n=n, wb=0) == E_WORKSPACE
    assert lib.rarc_merge_plan_workspace_bytes(0) == 0 == lib.rarc_merge_plan_workspace_bytes(N_LIMIT) and lib.rarc_merge_plan_workspace_bytes(1) > 0


def test_the_ranges_of_the_lists():
    lib = B.load_library()
    for m in (0, -1, 1 << 31):
        assert _pairs(lib, m=m) == E_INVALID and b"rarc_merge_pairs: m=" in lib.rarc_last_error() and lib.rarc_merge_pairs_workspace_bytes(m) == 0
        assert _mentions(lib, nnz=m) == E_INVALID and b"rarc_merge_mentions: nnz=" in lib.rarc_last_error()
        assert lib.rarc_merge_mentions_workspace_bytes(300, m) == 0
    for nc in (0, -1, N_LIMIT):
        assert _mentions(lib, nc=nc) == E_INVALID and b"rarc_merge_mentions: n_chunks=" in lib.rarc_last_error()
        assert lib.rarc_merge_mentions_workspace_bytes(nc, 5000) == 0
    for r in (0, -1, N_LIMIT, 1 << 40):
        assert _relations(lib, r=r) == E_INVALID and b"relation rows out of range" in lib.rarc_last_error()
        assert lib.rarc_merge_relations_workspace_bytes(r) == 0
    assert _pairs(lib, m=(1 << 31) - 1, n=N_LIMIT - 1, wb=0) == E_WORKSPACE           # 31 + 31 bits of key: inside the sort's 62
    assert _mentions(lib, nc=N_LIMIT - 1, nnz=(1 << 31) - 1, n=N_LIMIT - 1, wb=0) == E_WORKSPACE
    assert _relations(lib, r=N_LIMIT - 1, wb=0) == E_WORKSPACE


def test_short_workspaces_and_their_sizes():
    lib = B.load_library()
    need = lib.rarc_sort_reduce_workspace_bytes(1000)
    assert need >= 1000 * (2 * 8 + 2 * 4 + 2 * 4) and need % 256 == 0             # two key and value buffers, flags and positions
    assert _sort(lib, wb=need - 1) == E_WORKSPACE and b"rarc_sort_reduce: workspace of" in lib.rarc_last_error()
    assert lib.rarc_sort_reduce_workspace_bytes(100_000) > 50 * need
    for fn, size in ((_plan, lib.rarc_merge_plan_workspace_bytes(1000)), (_pairs, lib.rarc_merge_pairs_workspace_bytes(5000)),
                     (_mentions, lib.rarc_merge_mentions_workspace_bytes(300, 5000)), (_relations, lib.rarc_merge_relations_workspace_bytes(7000))):
        assert size > 0 and fn(lib, wb=size - 1) == E_WORKSPACE and b"workspace of" in lib.rarc_last_error()
    assert lib.rarc_merge_pairs_workspace_bytes(5000) > lib.rarc_sort_reduce_workspace_bytes(5000)
    assert lib.rarc_merge_mentions_workspace_bytes(30_000, 5000) > lib.rarc_merge_mentions_workspace_bytes(300, 5000)


def test_limits_agree_with_the_python_constants():
    from rag_arc_amd.encapsulation.database.graph_db import merge as M
    from rag_arc_amd.encapsulation.database.graph_db import passages

    assert M.limits() == {"tile": 2048, "radix_bits": 8, "max_key_bits": M.MAX_KEY_BITS, "max_count": M.MAX_COUNT}
    assert (M.MAX_KEY_BITS, M.MAX_COUNT, M.MAX_RICHNESS) == (62, 1 << 31, 1 << 32) and passages.MAX_MENTION_WEIGHT == 1 << 12
    assert B.load_library().rarc_sort_reduce_limits(None) == E_INVALID


def test_python_arguments_are_refused_before_a_device_is_needed():
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph, MentionMap, RelationList, merge_entities, merge_plan
    from rag_arc_amd.encapsulation.database.graph_db import merge as M

    for bad in ([], [[0, 1]], [0, 2], [-1, 0], [0.5, 0]):                             # empty, not a vector, outside [0, n), no integers
        with pytest.raises(ValueError):
            merge_plan(bad)
        with pytest.raises(ValueError):
            merge_entities(bad)
    for rich in ([1], [1, -1], [1, 1 << 32], [0.5, 1], [[1, 2]]):
        with pytest.raises(ValueError, match="richness"):
            merge_plan([0, 0], rich)
    for kw in ({"key_bits": 0}, {"key_bits": 63}, {"values": [1]}, {"values": [1, -1]}, {"values": [1, 1 << 32]}):
        with pytest.raises(ValueError):
            M.sort_reduce([1, 2], **kw)
    with pytest.raises(ValueError, match="keys"):
        M.sort_reduce([1, 256], key_bits=8)
    with pytest.raises(ValueError):
        M.sort_reduce([])
    # inputs over another number of entities, of another type or on another device: refused against the plan
    plan = M.MergePlan(3, 2, None, None, None, None, device="cuda:0", new_id_device=None)

    def fake(kind, n, device="cuda:0"):
        x = kind.__new__(kind)
        x.device = device
        setattr(x, "n" if kind is EntityGraph else "n_entities", n)
        return x

    for kind, kw in ((EntityGraph, "graph"), (MentionMap, "mentions"), (RelationList, "relations")):
        with pytest.raises(ValueError, match="4 entities"):
            merge_entities(plan, **{kw: fake(kind, 4)})
        with pytest.raises(ValueError, match="4 entities"):
            merge_entities([0, 0, 2], **{kw: fake(kind, 4)})
        with pytest.raises(ValueError, match="cuda:1"):
            merge_entities(plan, **{kw: fake(kind, 3, "cuda:1")})
        with pytest.raises(ValueError, match=kind.__name__):
            merge_entities(plan, **{kw: types.SimpleNamespace(n=3, n_entities=3, device="cuda:0")})
    with pytest.raises(ValueError, match="richness"):
        merge_entities(plan, richness=[1, 2, 3])
    M._check_inputs(plan, fake(EntityGraph, 3), fake(MentionMap, 3), fake(RelationList, 3))
    M._check_inputs(plan, None, None, None)


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import deduplicate_entities, merge_entities, merge_plan
    from rag_arc_amd.encapsulation.database.graph_db import merge as M

    if torch.cuda.is_available():
        plan = merge_plan([1, 1, 2], [0, 3, 0])
        assert plan.kept.tolist() == [1, 2] and plan.new_id.tolist() == [0, 0, 1] and merge_entities(plan).graph is None
        return
    for call in (lambda: merge_plan([1, 1, 2]), lambda: merge_entities([1, 1, 2]), lambda: M.sort_reduce([3, 1, 3]),
                 lambda: deduplicate_entities(np.eye(3, dtype=np.float32))):
        with pytest.raises(B.RarcError, match="no CPU fallback"):
            call()
