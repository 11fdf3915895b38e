"""The ingest entry points alone (rarc_ingest_pairs, rarc_ingest_mentions, their workspace sizes and limits; csrc/merge.hip, DESIGN
§4.13n) against the restatement tests/ingest_ref.py, element for element — nothing here is floating point.  Key widths of 2, 6, 18
and 34 bits cross one, three and five radix passes; row counts sit on both sides of a wave and of a 2048-key sort tile.  Every
output buffer is filled with a pattern first: no slot at or past the reported count may change.  Every case runs a second time
with its rows shuffled and must give the same bytes.  The refused shapes need no device: the pointers are never dereferenced."""
import ctypes

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: torch brings the HIP runtime both must share)

from rag_arc_amd.hip import binding as B
from tests import ingest_ref as R

gpu = pytest.mark.gpu
P = ctypes.c_void_p(4096)       # a non-null, 256-byte aligned pointer nobody reads
E_INVALID, E_WORKSPACE = -1, -3
BIG = 1 << 60
FILL = 0x5A


def _dev(a, dtype):
    a = np.ascontiguousarray(np.asarray(a).astype(dtype))
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _ptr(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _buffer(count, dtype, width=1):
    size = torch.empty(0, dtype=dtype).element_size()
    return torch.full((count * width * size,), FILL, dtype=torch.uint8, device="cuda").view(dtype)


def run_pairs(n, rows, w=None, t=None, bp=None, bw=None, bm=None, typed=None):
    """-> (pairs, weights or None, masks or None, out8 list, the untouched tails are asserted here)"""
    lib = B.load_library()
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    r, m0 = len(rows), 0 if bp is None else len(bp)
    cap = m0 + r
    typed = (t is not None or bm is not None) if typed is None else typed
    unit = w is None and bw is None
    d_rows, d_w, d_t = _dev(rows, np.int64), None if w is None else _dev(w, np.uint32), None if t is None else _dev(t, np.int32)
    d_bp = None if bp is None else _dev(np.asarray(bp, np.int64).reshape(-1, 2), np.int64)
    d_bw, d_bm = None if bw is None else _dev(bw, np.uint32), None if bm is None else _dev(bm, np.uint32)
    ws = torch.empty(int(lib.rarc_ingest_pairs_workspace_bytes(m0, r)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0 and ws.data_ptr() % 256 == 0
    op, ow, om = _buffer(cap, torch.int64, 2), _buffer(cap, torch.int32), _buffer(cap, torch.int32) if typed else None
    out8 = torch.empty(8, dtype=torch.int64, device="cuda")
    B.check(lib.rarc_ingest_pairs(_ptr(d_rows), _ptr(d_w), _ptr(d_t), r, _ptr(d_bp), _ptr(d_bw), _ptr(d_bm), m0, n, ws.data_ptr(), ws.numel(),
                                  op.data_ptr(), ow.data_ptr(), _ptr(om), out8.data_ptr(), None), "rarc_ingest_pairs")
    torch.cuda.synchronize()
    counts = out8.tolist()
    m = counts[0]
    assert 0 <= m <= cap
    op, ow = op.cpu().numpy().reshape(cap, 2), ow.cpu().numpy().view(np.uint32)
    pattern64, pattern32 = np.int64(int.from_bytes(bytes([FILL]) * 8, "little")), np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))
    assert np.all(op[m:] == pattern64) and np.all(ow[m:] == pattern32), "a slot past the reported count was written"
    if om is not None:
        om = om.cpu().numpy().view(np.uint32)
        assert np.all(om[m:] == pattern32), "a mask slot past the reported count was written"
        om = om[:m]
    return op[:m], ow[:m], om, counts, unit


def check_pairs(n, rows, w=None, t=None, bp=None, bw=None, bm=None, seed=0):
    want = R.ingest_pairs(n, rows, w, t, base_pairs=bp, base_weights=bw, base_masks=bm)
    got = run_pairs(n, rows, w, t, bp, bw, bm)
    pairs, weights, masks, counts, unit = got
    assert np.array_equal(pairs, want.pairs), (len(pairs), len(want.pairs))
    if unit:
        assert np.all(weights == 1)
    else:
        assert np.array_equal(weights, (want.weights & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert (masks is None) == (want.masks is None) and (masks is None or np.array_equal(masks, want.masks))
    assert counts[0] == want.edges and counts[1] & (2**64 - 1) == want.largest and counts[2] == want.total
    assert dict(zip(R.PAIR_KINDS, counts[3:7])) == want.skipped and counts[7] == want.base_skipped
    # the same rows in another order (and the base in another order): the same bytes
    rng = np.random.default_rng(seed + 1000)
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    p = rng.permutation(len(rows))
    q = None if bp is None else rng.permutation(len(bp))
    sub = lambda x, i: None if x is None else np.asarray(x)[i]          # noqa: E731
    again = run_pairs(n, rows[p], sub(w, p), sub(t, p), sub(bp, q), sub(bw, q), sub(bm, q), typed=masks is not None)
    assert again[0].tobytes() == pairs.tobytes() and again[1].tobytes() == weights.tobytes() and again[3] == counts
    assert masks is None or again[2].tobytes() == masks.tobytes()
    return want


def _mixed_rows(rng, n, r, bad=True):
    """r rows over n vertices in any orientation with duplicates; with `bad`, about one row in six is outside the rule"""
    a = rng.integers(0, n, r)
    b = rng.integers(0, n, r)
    w = rng.integers(1, 1000, r)
    t = rng.integers(0, 32, r)
    if bad:
        kind = rng.integers(0, 32, r)
        a = np.where(kind == 0, n + rng.integers(0, 3, r), a)
        b = np.where(kind == 1, -1 - rng.integers(0, 3, r), b)
        w = np.where(kind == 2, 0, w)
        t = np.where(kind == 3, 32 + rng.integers(0, 3, r), np.where(kind == 4, -1, t))
    return np.stack([a, b], axis=1).astype(np.int64), w, t


# ---- key widths x row counts ------------------------------------------------------------------------------------------------------------
ROW_COUNTS = (1, 63, 64, 65, 2047, 2048, 2049, 10000)


@gpu
@pytest.mark.parametrize("n", [2, 5, 300, 70000])
def test_key_widths_and_row_counts_typed_and_weighted(n):
    rng = np.random.default_rng(n)
    for r in ROW_COUNTS:
        rows, w, t = _mixed_rows(rng, n, r)
        check_pairs(n, rows, w, t, seed=r)


@gpu
@pytest.mark.parametrize("n", [2, 5, 300, 70000])
def test_key_widths_and_row_counts_untyped_and_unit(n):
    rng = np.random.default_rng(n + 7)
    for r in ROW_COUNTS:
        rows, w, _ = _mixed_rows(rng, n, r)
        check_pairs(n, rows, seed=r)
        if r in (65, 2049):
            check_pairs(n, rows, w, seed=r)


# ---- long runs and large weights --------------------------------------------------------------------------------------------------------
@gpu
def test_a_run_of_one_pair_across_waves_and_tiles_and_a_sum_past_32_bits():
    rows = np.tile([[7, 3], [3, 7]], (2500, 1))
    want = check_pairs(300, rows, np.full(5000, 3), np.arange(5000) % 32)
    assert want.edges == 1 and want.weights.tolist() == [15000] and want.masks.tolist() == [0xFFFFFFFF]
    heavy = check_pairs(300, rows, np.full(5000, 1 << 20))
    assert heavy.largest == 5000 << 20 > 1 << 32 and heavy.total == heavy.largest                  # reported in 64 bits, not wrapped
    top = check_pairs(300, [[1, 2], [2, 1], [0, 1]], [(1 << 32) - 1, (1 << 32) - 1, 5])
    assert top.largest == (1 << 33) - 2


# ---- rows that yield no edge; orientation; self-loops -----------------------------------------------------------------------------------
@gpu
def test_every_row_invalid_gives_no_edge_and_writes_no_slot():
    rows = [[0, 5], [5, 0], [-1, 2], [3, 3], [0, 0], [1, 2], [2, 1], [1, 3]]
    want = check_pairs(5, rows, [1, 1, 1, 1, 1, 0, 0, 4], [0, 0, 0, 0, 0, 0, 0, 32])
    assert want.edges == 0 and want.skipped == {"out_of_range": 3, "self_loop": 2, "zero_weight": 2, "bad_type": 1}
    assert (want.largest, want.total) == (0, 0)
    assert check_pairs(5, [[0, 0]] * 70).skipped["self_loop"] == 70                                  # self-loops only, unit mode
    assert check_pairs(5, [[4, 4], [0, 0], [2, 2]], [1, 2, 3]).edges == 0


@gpu
def test_both_orientations_of_one_pair_are_one_edge():
    want = check_pairs(70000, [[69999, 0], [0, 69999]], [2, 3], [4, 9])
    assert want.pairs.tolist() == [[0, 69999]] and want.weights.tolist() == [5] and want.masks.tolist() == [(1 << 4) | (1 << 9)]
    assert check_pairs(2, [[1, 0], [0, 1], [1, 0]]).pairs.tolist() == [[0, 1]]
    # the pair (0, 1) has the smallest key a real edge can have: it must survive beside skipped rows, which take key 0
    assert check_pairs(300, [[1, 0], [5, 5], [400, 1]], [6, 1, 1]).weights.tolist() == [6]


# ---- types --------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_types_at_both_ends_all_of_them_and_outside():
    assert check_pairs(5, [[1, 2], [2, 1]], [1, 1], [0, 31]).masks.tolist() == [(1 << 31) | 1]
    all32 = check_pairs(300, [[10, 20]] * 32, np.ones(32, np.int64), np.arange(32))
    assert all32.masks.tolist() == [0xFFFFFFFF] and all32.weights.tolist() == [32]
    out = check_pairs(5, [[1, 2], [1, 2], [1, 2], [3, 4]], [1, 1, 1, 1], [32, -1, 5, -(1 << 31)])
    assert out.skipped["bad_type"] == 3 and out.masks.tolist() == [1 << 5] and out.weights.tolist() == [1]


# ---- bases --------------------------------------------------------------------------------------------------------------------------------
def _base(rng, n, m, weighted=True, typed=True):
    keys = rng.choice(n * n, size=4 * m, replace=False)
    i, j = keys // n, keys % n
    keep = i < j
    bp = np.stack([i[keep], j[keep]], axis=1)[:m].astype(np.int64)
    return bp, (rng.integers(1, 100, len(bp)) if weighted else None), (rng.integers(0, 1 << 32, len(bp), dtype=np.uint64).astype(np.uint32) if typed else None)


@gpu
def test_a_base_in_descending_order_overlapping_the_new_rows():
    rng = np.random.default_rng(41)
    n = 300
    bp, bw, bm = _base(rng, n, 3000)
    order = np.lexsort((bp[:, 1], bp[:, 0]))[::-1]                      # descending by (i, j)
    bp, bw, bm = bp[order], bw[order], bm[order]
    rows, w, t = _mixed_rows(rng, n + 50, 2500)
    rows[:500] = bp[:500, ::-1]                                         # 500 new rows name resident pairs, the other way round
    want = check_pairs(n + 50, rows, w, t, bp, bw, bm)
    assert want.edges > len(bp) and want.base_skipped == 0
    # every combination of a weighted and an unweighted side; untyped
    for base_weighted, rows_weighted in ((True, False), (False, True), (False, False)):
        check_pairs(n + 50, rows, w if rows_weighted else None, None, bp, bw if base_weighted else None, None)


@gpu
def test_an_empty_base_a_base_alone_and_a_damaged_base():
    rng = np.random.default_rng(43)
    rows, w, t = _mixed_rows(rng, 300, 700, bad=False)
    a = check_pairs(300, rows, w, t)
    b = check_pairs(300, rows, w, t, np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint32))
    assert a.pairs.tobytes() == b.pairs.tobytes() and a.masks.tobytes() == b.masks.tobytes()
    # the result as a base with no new row: itself
    again = check_pairs(300, np.zeros((0, 2), np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64), a.pairs, a.weights, a.masks)
    assert again.pairs.tobytes() == a.pairs.tobytes() and again.weights.tobytes() == a.weights.tobytes() and again.masks.tobytes() == a.masks.tobytes()
    damaged = check_pairs(5, [[0, 1]], [1], [2], [[0, 1], [2, 1], [3, 3], [1, 5], [-1, 2], [2, 4]], [4, 1, 1, 1, 1, 0], [1, 1, 1, 1, 1, 1])
    assert damaged.base_skipped == 5 and damaged.pairs.tolist() == [[0, 1]] and damaged.weights.tolist() == [5] and damaged.masks.tolist() == [5]


@gpu
def test_unit_mode_against_the_weighted_mode_on_the_same_rows():
    rng = np.random.default_rng(47)
    rows, _, t = _mixed_rows(rng, 300, 5000)
    unit = check_pairs(300, rows, None, t)
    ones = check_pairs(300, rows, np.ones(5000, np.int64), t)
    assert unit.pairs.tobytes() == ones.pairs.tobytes() and unit.masks.tobytes() == ones.masks.tobytes() and unit.weights is None
    assert ones.largest > 1 and unit.largest == 1 and unit.total == unit.edges and ones.total == int(ones.weights.sum())


# ---- mentions -----------------------------------------------------------------------------------------------------------------------------
def run_mentions(n_chunks, n_entities, rows, w=None, base=None):
    lib = B.load_library()
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    r = len(rows)
    nnz0, base_chunks = (0, 0) if base is None else (len(base[1]), len(base[0]) - 1)
    cap = nnz0 + r
    d_rows, d_w = _dev(rows, np.int64), None if w is None else _dev(w, np.uint32)
    d_base = (None, None, None) if base is None else (_dev(base[0], np.int64), _dev(base[1], np.int32), _dev(base[2], np.uint32))
    ws = torch.empty(int(lib.rarc_ingest_mentions_workspace_bytes(n_chunks, nnz0, r)), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0
    orp, oe, ow, osp = _buffer(n_chunks + 1, torch.int64), _buffer(cap, torch.int32), _buffer(cap, torch.int32), _buffer(n_chunks, torch.int32)
    out8 = torch.empty(8, dtype=torch.int64, device="cuda")
    B.check(lib.rarc_ingest_mentions(_ptr(d_rows), _ptr(d_w), r, *(_ptr(x) for x in d_base), base_chunks, nnz0, n_chunks, n_entities, ws.data_ptr(),
                                     ws.numel(), orp.data_ptr(), oe.data_ptr(), ow.data_ptr(), osp.data_ptr(), out8.data_ptr(), None),
            "rarc_ingest_mentions")
    torch.cuda.synchronize()
    counts = out8.tolist()
    nnz, n_split = counts[0], counts[2]
    pattern32 = np.uint32(int.from_bytes(bytes([FILL]) * 4, "little"))
    oe, ow, osp = oe.cpu().numpy(), ow.cpu().numpy().view(np.uint32), osp.cpu().numpy()
    assert np.all(oe[nnz:].view(np.uint32) == pattern32) and np.all(ow[nnz:] == pattern32) and np.all(osp[n_split:].view(np.uint32) == pattern32)
    return orp.cpu().numpy(), oe[:nnz], ow[:nnz], osp[:n_split], counts


def check_mentions(n_chunks, n_entities, rows, w=None, base=None, seed=0):
    want = R.ingest_mentions(n_chunks, n_entities, rows, w, base=base)
    got = run_mentions(n_chunks, n_entities, rows, w, base)
    assert np.array_equal(got[0], want.row_ptr) and np.array_equal(got[1], want.entities)
    assert np.array_equal(got[2], (want.weights & np.uint64(0xFFFFFFFF)).astype(np.uint32)) and np.array_equal(got[3], want.split)
    counts = got[4]
    assert (counts[0], counts[1], counts[2]) == (want.nnz, want.largest, len(want.split))
    assert dict(zip(R.MENTION_KINDS, counts[3:6])) == want.skipped and counts[6] == 0 and counts[7] == want.base_skipped
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    p = np.random.default_rng(seed + 2000).permutation(len(rows))
    again = run_mentions(n_chunks, n_entities, rows[p], None if w is None else np.asarray(w)[p], base)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:4], again[:4])) and again[4] == counts
    return want


def _chunk_rows(degrees, n_entities, rng):
    rows = [(c, e) for c, d in enumerate(degrees) for e in rng.choice(n_entities, size=d, replace=False)]
    return np.array(rows, np.int64).reshape(-1, 2)


@gpu
def test_mention_chunks_of_every_degree_around_the_split_and_trailing_empty_chunks():
    rng = np.random.default_rng(51)
    split = B.load_library()
    out = (ctypes.c_int * 4)()
    assert split.rarc_ingest_limits(out) == 0 and list(out) == [32, 12, 64, 31]
    degrees = [3, 0, 64, 65, 1, 200, 0, 0]                              # 0 mentions, exactly the split degree, one more; two trailing empty
    rows = _chunk_rows(degrees, 300, rng)
    rows = np.concatenate([rows, rows[::3]])                            # duplicates add up without changing a degree
    w = rng.integers(1, 20, len(rows))
    want = check_mentions(len(degrees), 300, rows, w)
    assert np.diff(want.row_ptr).tolist() == degrees and want.split.tolist() == [3, 5]
    check_mentions(len(degrees), 300, rows)                             # unit weights
    one = check_mentions(4, 1, [[0, 0], [2, 0], [2, 0], [3, 1], [4, 0]], [5, 1, 2, 1, 1])          # n_entities = 1
    assert one.entities.tolist() == [0, 0] and one.weights.tolist() == [5, 3] and one.skipped["entity_out_of_range"] == 1
    assert one.skipped["chunk_out_of_range"] == 1 and one.row_ptr.tolist() == [0, 1, 1, 2, 2]


@gpu
def test_mention_key_zero_beside_skipped_rows_and_with_no_valid_row_at_all():
    # a skipped row takes the key of (chunk 0, entity 0) with value 0: the real mention (0, 0) must keep its own sum ...
    kept = check_mentions(3, 3, [[0, 0], [9, 9], [0, 0], [1, 2], [0, 7]], [2, 1, 3, 1, 1])
    assert kept.row_ptr.tolist() == [0, 1, 2, 2] and kept.weights.tolist() == [5, 1]
    # ... and without one the key must not appear
    absent = check_mentions(3, 3, [[9, 9], [1, 2], [0, 7]], [1, 1, 1])
    assert absent.row_ptr.tolist() == [0, 0, 1, 1] and absent.entities.tolist() == [2]
    nothing = check_mentions(3, 3, [[9, 9], [0, 7], [1, 1]], [1, 1, 0])
    assert nothing.nnz == 0 and nothing.row_ptr.tolist() == [0, 0, 0, 0] and nothing.largest == 0


@gpu
def test_a_summed_mention_weight_of_4095_and_of_4096():
    under = check_mentions(2, 5, [[1, 3]] * 4095)
    assert under.largest == 4095 and under.weights.tolist() == [4095]
    over = check_mentions(2, 5, [[1, 3], [1, 3], [1, 3]], [4095, 1, 4096])
    assert over.largest == 4096 and over.skipped["bad_weight"] == 1    # the device's own maximum: the caller's to refuse


@gpu
@pytest.mark.parametrize("n_entities, r", [(1, 65), (300, 2049), (70000, 10000)])
def test_a_mention_extension_that_adds_chunks_and_entities(n_entities, r):
    from rag_arc_amd.encapsulation.database.graph_db.passages import mention_csr

    rng = np.random.default_rng(r)
    n_chunks = 500
    first = np.stack([rng.integers(0, n_chunks, 3000), rng.integers(0, n_entities, 3000)], axis=1)
    base = mention_csr(n_chunks, n_entities, first, rng.integers(1, 5, 3000))[:3]
    rows = np.stack([rng.integers(-2, n_chunks + 40, r), rng.integers(-2, n_entities + 9, r)], axis=1)
    w = rng.integers(1, 6, r)
    rows[:6] = [[-1, 0], [n_chunks + 40, 0], [0, -1], [0, n_entities + 9], [n_chunks + 39, n_entities + 8], [1, 0]]
    w[4:6] = [0, 4096]                                                  # every kind at least once, whatever r
    want = check_mentions(n_chunks + 40, n_entities + 9, rows, w, base=base)
    assert want.base_skipped == 0 and all(want.skipped.values()) and want.row_ptr[-1] == want.nnz > len(base[1])
    # a damaged base: a row_ptr that runs past nnz, an entity out of range, a weight of 0 and of 2^12
    row_ptr, ent, bw = base[0].copy(), base[1].copy(), base[2].copy()
    row_ptr[-1] += 5
    ent[0], bw[1], bw[2] = n_entities + 20, 0, 4096
    assert check_mentions(n_chunks + 40, n_entities + 9, rows, w, base=(row_ptr, ent, bw)).base_skipped == 3


# ---- refused shapes: the project's error code, no launch -----------------------------------------------------------------------------------
def _pairs(lib, rows=P, w=P, t=P, r=1000, bp=P, bw=P, bm=P, m0=500, n=300, ws=P, wb=BIG, op=P, ow=P, om=P, out8=P):
    return lib.rarc_ingest_pairs(rows, w, t, r, bp, bw, bm, m0, n, ws, wb, op, ow, om, out8, None)


def _mentions(lib, rows=P, w=P, r=1000, brp=P, be=P, bw=P, bc=50, nnz0=500, nc=80, ne=300, ws=P, wb=BIG, orp=P, oe=P, ow=P, osp=P, out8=P):
    return lib.rarc_ingest_mentions(rows, w, r, brp, be, bw, bc, nnz0, nc, ne, ws, wb, orp, oe, ow, osp, out8, None)


def test_version_is_unchanged_and_every_symbol_is_bound():
    lib = B.load_library()
    assert lib.rarc_version() == 600
    for name in ("rarc_ingest_pairs", "rarc_ingest_pairs_workspace_bytes", "rarc_ingest_mentions", "rarc_ingest_mentions_workspace_bytes",
                 "rarc_ingest_limits"):
        assert name in B.SIGNATURES and getattr(lib, name)
    assert lib.rarc_ingest_limits(None) == E_INVALID


def test_null_and_misaligned_pointers_are_refused():
    lib = B.load_library()
    for arg in ("rows", "bp", "ws", "op", "ow", "out8"):
        assert _pairs(lib, **{arg: None}) == E_INVALID and b"rarc_ingest_pairs: null pointer" in lib.rarc_last_error(), arg
    for arg in ("rows", "brp", "be", "bw", "ws", "orp", "oe", "ow", "osp", "out8"):
        assert _mentions(lib, **{arg: None}) == E_INVALID and b"rarc_ingest_mentions: null pointer" in lib.rarc_last_error(), arg
    # a side of length 0 may pass null pointers; unit mode needs no weight output; untyped needs no types
    assert _pairs(lib, rows=None, w=None, t=None, r=0, wb=0) == E_WORKSPACE and _pairs(lib, bp=None, bw=None, bm=None, m0=0, wb=0) == E_WORKSPACE
    assert _pairs(lib, w=None, bw=None, ow=None, wb=0) == E_WORKSPACE and _pairs(lib, t=None, bm=None, om=None, wb=0) == E_WORKSPACE
    assert _mentions(lib, brp=None, be=None, bw=None, bc=0, nnz0=0, wb=0) == E_WORKSPACE and _mentions(lib, w=None, wb=0) == E_WORKSPACE
    # typed and untyped sides mixed
    for kw in ({"t": None}, {"bm": None}, {"om": None}, {"om": None, "t": None}):
        assert _pairs(lib, **kw) == E_INVALID and b"typed and untyped" in lib.rarc_last_error(), kw
    odd = lambda a: ctypes.c_void_p(4096 + a)                          # noqa: E731
    assert _pairs(lib, ws=odd(128)) == E_INVALID and b"rarc_ingest_pairs: the workspace is not 256-byte aligned" in lib.rarc_last_error()
    assert _mentions(lib, ws=odd(128)) == E_INVALID and b"rarc_ingest_mentions: the workspace is not 256-byte aligned" in lib.rarc_last_error()
    for arg in ("rows", "w", "t", "bp", "bw", "bm", "op", "ow", "om", "out8"):
        assert _pairs(lib, **{arg: odd(2)}) == E_INVALID and b"rarc_ingest_pairs: an array is not aligned" in lib.rarc_last_error(), arg
    for arg in ("rows", "w", "brp", "be", "bw", "orp", "oe", "ow", "osp", "out8"):
        assert _mentions(lib, **{arg: odd(2)}) == E_INVALID and b"rarc_ingest_mentions: an array is not aligned" in lib.rarc_last_error(), arg


def test_the_count_and_vertex_limits():
    lib = B.load_library()
    top = (1 << 31) - 1
    for m0, r in ((1 << 30, 1 << 30), (top, 1), (0, 1 << 31), (0, 0), (-1, 5), (5, -1)):              # m0 + r = 2^31 and beyond; nothing; negative
        assert _pairs(lib, m0=m0, r=r) == E_INVALID and b"rarc_ingest_pairs: m0=" in lib.rarc_last_error()
        assert lib.rarc_ingest_pairs_workspace_bytes(m0, r) == 0
        assert _mentions(lib, nnz0=m0, r=r) == E_INVALID and b"rarc_ingest_mentions: nnz0=" in lib.rarc_last_error()
        assert lib.rarc_ingest_mentions_workspace_bytes(80, m0, r) == 0
    assert _pairs(lib, m0=top - 1, r=1, n=top - 1, wb=0) == E_WORKSPACE and lib.rarc_ingest_pairs_workspace_bytes(top - 1, 1) > 0
    for n in (1, 0, -1, top, 1 << 40):
        assert _pairs(lib, n=n) == E_INVALID and f"rarc_ingest_pairs: n={n} out of range".encode() in lib.rarc_last_error()
    assert _pairs(lib, n=2, wb=0) == E_WORKSPACE
    for nc in (0, -1, top):
        assert _mentions(lib, nc=nc) == E_INVALID and b"rarc_ingest_mentions: n_chunks=" in lib.rarc_last_error()
        assert lib.rarc_ingest_mentions_workspace_bytes(nc, 500, 1000) == 0
    for ne in (0, -1, top):
        assert _mentions(lib, ne=ne) == E_INVALID and b"rarc_ingest_mentions: n_entities=" in lib.rarc_last_error()
    for bc in (0, -1, 81):
        assert _mentions(lib, bc=bc) == E_INVALID and b"rarc_ingest_mentions: base_chunks=" in lib.rarc_last_error()
    assert _mentions(lib, nc=top - 1, ne=top - 1, bc=top - 1, nnz0=top - 1, r=1, wb=0) == E_WORKSPACE
    need = lib.rarc_ingest_pairs_workspace_bytes(500, 1000)
    assert need % 256 == 0 and need > lib.rarc_sort_reduce_workspace_bytes(1500) and _pairs(lib, wb=need - 1) == E_WORKSPACE
    assert b"rarc_ingest_pairs: workspace of" in lib.rarc_last_error()
    need = lib.rarc_ingest_mentions_workspace_bytes(80, 500, 1000)
    assert need > lib.rarc_sort_reduce_workspace_bytes(1500) and _mentions(lib, wb=need - 1) == E_WORKSPACE
    assert lib.rarc_ingest_mentions_workspace_bytes(80_000, 500, 1000) > need
