"""rarc_mmr_select_rows (csrc/fuse.hip) through the C ABI: the batched MMR selection that reads its candidates from an index's
resident rows.  For every query two things are asked of its picks:
  (a) they equal rarc_mmr_select's — the single-query kernel — on the same candidates gathered to fp32 as the store gathers
      them, index for index (the arithmetic contract: same sequential float64 sums);
  (b) rank_ref.mmr_check_walk passes: each pick within the derived rounding bound of the longdouble best, the lowest index among
      exactly equal candidates.
Inputs are rank_ref.mmr_inputs over rank_ref.mmr_cases (test_rank_ref_host.py keeps their near-ties rare) stacked into ONE
metric-"ip" index per (storage, d): no normalisation at add, and the 1/128 grid is exact in fp16 and fp32.  Every query owns a
contiguous id range, its list padded with -1 to the widest n; the index has a non-zero id_base.  Reference picks are computed
once per case and shared by the storages (their gathered candidates are the same fp32 numbers, which the test asserts)."""
import numpy as np
import pytest

from tests import rank_ref as R

pytestmark = pytest.mark.gpu

NS = (1, 2, 255, 257, 1024)
DS = (3, 64, 768)
ID_BASE = 7_000_000_000          # (beyond 2^32: ids are 64-bit all the way)
FMT = {"f16": 0, "f8": 1, "f32": 2}


def _lib():
    from rag_arc_amd.hip import binding as B

    return B, B.load_library()


def _select_rows(idx, queries, cand_ids, normalize, k, lam):
    """One rarc_mmr_select_rows call: queries float64 [nq][dim], cand_ids int64 [nq][n] -> int64 [nq][k] (pre-filled with -7)."""
    import torch

    B, lib = _lib()
    q = torch.from_numpy(np.ascontiguousarray(queries, np.float64)).cuda()
    ids = torch.from_numpy(np.ascontiguousarray(cand_ids, np.int64)).cuda()
    nq, n = ids.shape
    nbytes = int(lib.rarc_mmr_rows_workspace_bytes(nq, n, idx.dim))
    assert nbytes == nq * (n * idx.dim + idx.dim) * 8
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    scales = idx._rowscale.data_ptr() if idx.storage == "f8" else 0
    B.check(lib.rarc_mmr_select_rows(idx._rows.data_ptr(), FMT[idx.storage], scales, idx.ntotal, idx.d_pad, idx.dim, q.data_ptr(),
                                     q.shape[1], nq, ids.data_ptr(), n, idx.id_base, int(normalize), int(k), float(lam),
                                     out.data_ptr(), ws.data_ptr(), nbytes, 0), "rarc_mmr_select_rows")
    return out.cpu().numpy()


def _gathered(idx, rows):
    """The candidates as HipFlatVectorStore._mmr_on_device gathers them: fp32 [n][dim] on the device."""
    import torch

    sel = torch.as_tensor(np.asarray(rows, np.int64), device=idx.rows.device)
    r = idx.rows[sel]
    if idx.storage == "f8":
        cand = r.view(torch.float8_e4m3fn).to(torch.float32) * idx.row_scales[sel][:, None]
    else:
        cand = r.to(torch.float32)
    return cand[:, : idx.dim].contiguous()


def _select_one(cand, query, normalize, k, lam):
    """rarc_mmr_select (the single-query kernel) over gathered candidates: its min(k, n) picks."""
    import torch

    B, lib = _lib()
    n, d = cand.shape
    q = torch.from_numpy(np.ascontiguousarray(query, np.float64)).cuda()
    work = torch.empty(int(lib.rarc_mmr_workspace_doubles(n, d)), dtype=torch.float64, device="cuda")
    out = torch.full((min(k, n),), -7, dtype=torch.int32, device="cuda")
    B.check(lib.rarc_mmr_select(cand.data_ptr(), d, q.data_ptr(), n, d, int(normalize), int(k), float(lam), work.data_ptr(),
                                out.data_ptr(), 0), "rarc_mmr_select")
    return out.cpu().numpy().tolist()


# ---- the stacked index of one (storage, d): every n of NS x the sixteen variants of rank_ref.mmr_cases --------------------------
_STACKS: dict = {}
_REF_PICKS: dict = {}          # (d, n, variant, k) -> rarc_mmr_select's picks: shared by the storages
_WALKED: set = set()           # (d, n, variant, picks) that mmr_check_walk has passed


def _stack(storage, d):
    """(index, {(n, lam, nm, ties): (first row, cand fp32, query fp64)})."""
    if (storage, d) not in _STACKS:
        from rag_arc_amd.hip.engine import FlatIndexF16

        where, blocks, at = {}, [], 0
        for n in NS:
            for lam, nm, ties, seed in R.mmr_cases(n, d):
                cand, q = R.mmr_inputs(n, d, seed, ties)
                where[(n, lam, nm, ties)] = (at, cand, q)
                blocks.append(cand)
                at += n
        idx = FlatIndexF16(d, metric="ip", device=0, storage=storage, id_base=ID_BASE)
        idx.add(np.concatenate(blocks))
        assert idx.ntotal == at and (d < idx.d_pad) == (d % 128 != 0)
        _STACKS[(storage, d)] = (idx, where)
    return _STACKS[(storage, d)]


def _rewound(ref, lam):
    """An MMRRef back at its start (candidate 0 taken) for another walk, with another lambda if asked: the exact similarities
    it holds do not depend on either (nor does its tolerance: rank_ref.mmr_tol)."""
    ref.lam, ref.one_minus = R.LD(lam), R.LD(1.0) - R.LD(lam)
    ref.taken[:] = False
    ref.maxsim[:] = 0
    ref.take(0)
    return ref


_REFS: dict = {}               # (d, n, variant) -> MMRRef, for the test case that is running


def _check_query(idx, d, n, variant, first, cand, q, k, got):
    """(a) and (b) for one query's output row `got` (int64 [k])."""
    lam, nm, ties = variant
    what = f"storage={idx.storage} d={d} n={n} lam={lam} normalize={nm} ties={ties} k={k}"
    take = min(k, n)
    assert (got[take:] == -1).all(), what
    picks = (got[:take] - ID_BASE - first).tolist()
    key = (d, n, variant, k)
    if key not in _REF_PICKS:
        gathered = _gathered(idx, np.arange(first, first + n))
        assert np.array_equal(gathered.cpu().numpy(), cand), what        # (the grid is exact in this storage)
        # (the single-query kernel has no k >= n short cut of its own: the store returns the given order there)
        _REF_PICKS[key] = list(range(n)) if k >= n else _select_one(gathered, q, nm, k, lam)
    assert picks == _REF_PICKS[key], what                                  # (a)
    if (d, n, variant, tuple(picks)) not in _WALKED:
        if (d, n, variant) not in _REFS:
            _REFS[(d, n, variant)] = R.MMRRef(cand, q, nm, lam)
        R.mmr_check_walk(_rewound(_REFS[(d, n, variant)], lam), picks, what)          # (b)
        _WALKED.add((d, n, variant, tuple(picks)))


@pytest.mark.parametrize("lam", R.MMR_LAMBDAS)
@pytest.mark.parametrize("nm", [0, 1])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_picks_equal_the_single_query_kernel_and_walk_the_reference(storage, d, nm, lam):
    """k = 1 and k = 5: ONE launch each holds every n (ten queries of 1 .. 1024 candidates side by side, the short ones
    padded with -1; n <= k gives the identity).  k = n - 1: one launch per n (two queries: without and with built ties)."""
    idx, where = _stack(storage, d)
    _REFS.clear()
    mine = [(n, ties) for n in NS for ties in (False, True)]
    width = max(NS)
    ids = np.full((len(mine), width), -1, np.int64)
    qs = np.empty((len(mine), d), np.float64)
    for row, (n, ties) in enumerate(mine):
        first, _, q = where[(n, lam, nm, ties)]
        ids[row, :n] = ID_BASE + first + np.arange(n)
        qs[row] = q
    for k in (1, 5):
        out = _select_rows(idx, qs, ids, nm, k, lam)
        for row, (n, ties) in enumerate(mine):
            first, cand, q = where[(n, lam, nm, ties)]
            _check_query(idx, d, n, (lam, nm, ties), first, cand, q, k, out[row])
    for n in NS:
        k = n - 1
        if k < 1 or k in (1, 5):
            continue
        rows = [r for r, (n_, _) in enumerate(mine) if n_ == n]
        out = _select_rows(idx, qs[rows], ids[rows], nm, k, lam)
        for o, r in zip(out, rows):
            first, cand, q = where[(n, lam, nm, mine[r][1])]
            _check_query(idx, d, n, (lam, nm, mine[r][1]), first, cand, q, k, o)


@pytest.mark.parametrize("n,k", [(20, 2), (20, 3), (20, 19), (64, 9), (64, 10), (64, 63), (65, 64), (256, 255)])
@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_both_sides_of_the_gram_threshold(storage, n, k):
    """Up to 64 candidates the pairwise similarities are formed before the rounds when that takes fewer passes than the rounds
    would (n = 20: from k = 3; n = 64: from k = 10), otherwise round by round; 256 / 257 candidates is where a thread starts to
    carry four sums.  Same picks as the single-query kernel on either side."""
    from rag_arc_amd.hip.engine import FlatIndexF16

    d = 64
    idx = FlatIndexF16(d, metric="ip", device=0, storage=storage, id_base=ID_BASE)
    cases = [(lam, nm, ties) for lam in (0.3, 0.5) for nm in (0, 1) for ties in (False, True)]
    inputs = [R.mmr_inputs(n, d, 40 + i, ties) for i, (_, _, ties) in enumerate(cases)]
    idx.add(np.concatenate([c for c, _ in inputs]))
    for i, (lam, nm, ties) in enumerate(cases):
        cand, q = inputs[i]
        ids = ID_BASE + i * n + np.arange(n)[None, :]
        got = _select_rows(idx, q[None, :], ids, nm, k, lam)[0]
        want = _select_one(_gathered(idx, ids[0] - ID_BASE), q, nm, k, lam)
        assert (got - ID_BASE - i * n).tolist() == want, (n, k, lam, nm, ties)
        R.mmr_check_walk(R.MMRRef(cand, q, nm, lam), want, f"n={n} k={k} lam={lam} normalize={nm} ties={ties}")


@pytest.mark.parametrize("n", [2, 20])
def test_fp8_rows(n):
    """Gaussian rows stored as e4m3fn bytes with a scale per row: the candidates are the decoded bytes times the scale, formed
    in fp32 — (a) against the single-query kernel on the gathered copy, (b) against the longdouble reference over exact
    products (rank_ref.exact_dots' Fraction path, hence the small shape)."""
    from rag_arc_amd.hip.engine import FlatIndexF16

    d = 256
    rng = np.random.default_rng([n, d, 8])
    idx = FlatIndexF16(d, metric="ip", device=0, storage="f8", id_base=ID_BASE)
    groups = 2
    idx.add((rng.standard_normal((groups * n, d)) * rng.uniform(0.2, 3.0, (groups * n, 1))).astype(np.float32))
    qs = rng.standard_normal((groups, d))
    ids = ID_BASE + np.arange(groups * n).reshape(groups, n)
    gathered = [_gathered(idx, ids[g] - ID_BASE) for g in range(groups)]
    hosts = [g.cpu().numpy() for g in gathered]
    assert all(np.unique(h).size > 16 for h in hosts)
    for nm in (0, 1):
        refs = [R.MMRRef(hosts[g], qs[g], nm, 0.5) for g in range(groups)]          # (the exact Gram matrices: built once)
        for lam in R.MMR_LAMBDAS:
            for k in sorted({1, 5, n - 1} - {0}):
                out = _select_rows(idx, qs, ids, nm, k, lam)
                for g in range(groups):
                    what = f"fp8 n={n} group={g} lam={lam} normalize={nm} k={k}"
                    take = min(k, n)
                    picks = (out[g, :take] - ID_BASE - g * n).tolist()
                    assert (out[g, take:] == -1).all(), what
                    want = list(range(n)) if k >= n else _select_one(gathered[g], qs[g], nm, k, lam)
                    assert picks == want, what
                    R.mmr_check_walk(_rewound(refs[g], lam), picks, what)


def _small_index(n_rows=400, d=64, storage="f16", seed=3):
    from rag_arc_amd.hip.engine import FlatIndexF16

    cand, _ = R.mmr_inputs(n_rows, d, seed, False)
    idx = FlatIndexF16(d, metric="ip", device=0, storage=storage, id_base=ID_BASE)
    idx.add(cand)
    return idx, cand


def test_k_at_least_the_candidates_gives_them_in_their_given_order():
    idx, _ = _small_index()
    rng = np.random.default_rng(11)
    ids = np.full((4, 30), -1, np.int64)
    counts = [30, 12, 1, 5]
    for r, c in enumerate(counts):
        ids[r, :c] = ID_BASE + rng.permutation(400)[:c]              # (any order: it is the GIVEN order that comes back)
    qs = rng.standard_normal((4, 64))
    for k in (30, 31, 64):
        out = _select_rows(idx, qs, ids, 1, k, 0.5)
        for r, c in enumerate(counts):
            assert out[r, :c].tolist() == ids[r, :c].tolist() and (out[r, c:] == -1).all(), (k, r)
    out = _select_rows(idx, qs, ids, 1, 12, 0.5)                      # k = 12: identity for the lists of 12, 1 and 5 only
    for r in (1, 2, 3):
        assert out[r, : counts[r]].tolist() == ids[r, : counts[r]].tolist() and (out[r, counts[r]:] == -1).all()
    assert out[0, 0] == ids[0, 0] and len(set(out[0].tolist())) == 12 and set(out[0].tolist()) <= set(ids[0].tolist())


def test_entries_that_name_no_row_are_skipped():
    """A list of nothing but -1 answers nothing but -1; ids below id_base or beyond the last row, and -1 in the middle of a
    list, are dropped before a row is read: the picks are those of the remaining candidates in their order."""
    idx, _ = _small_index()
    rng = np.random.default_rng(12)
    good = ID_BASE + rng.permutation(400)[:20]
    ids = np.full((3, 28), -1, np.int64)
    ids[1, :20] = good
    ids[2, [0, 3, 9, 27]] = [ID_BASE - 1, -1, ID_BASE + 400, 5]          # (5 < id_base: a row number, not an id)
    ids[2, [i for i in range(28) if i not in (0, 3, 9, 27)][:20]] = good
    qs = np.repeat(rng.standard_normal((1, 64)), 3, axis=0)
    out = _select_rows(idx, qs, ids, 1, 6, 0.5)
    assert (out[0] == -1).all()
    want = _select_one(_gathered(idx, good - ID_BASE), qs[1], 1, 6, 0.5)
    assert out[1].tolist() == good[want].tolist()
    assert out[2].tolist() == out[1].tolist()


def test_a_zero_row_under_normalize_picks_as_the_single_query_kernel():
    """A zero candidate normalises to NaN and never compares above anything: it is taken when nothing else is left, lowest
    index first — in the position the single-query kernel gives it."""
    import torch

    idx, cand = _small_index(n_rows=300)
    zeros = [3, 77, 256, 299]
    with torch.no_grad():
        idx._rows[zeros] = 0
    rows = np.arange(300)
    q = R.mmr_inputs(300, 64, 3, False)[1]
    for k in (5, 296, 298, 299):
        got = _select_rows(idx, q[None, :], ID_BASE + rows[None, :], 1, k, 0.5)[0]
        want = _select_one(_gathered(idx, rows), q, 1, k, 0.5)
        assert (got - ID_BASE).tolist() == want, k
    assert set(want[-3:]) <= set(zeros) and not set(want[:296]) & set(zeros)
    # a zero row FIRST in the list: every similarity to the first pick is NaN
    rows = np.array([77] + [i for i in range(40) if i != 3])
    got = _select_rows(idx, q[None, :], ID_BASE + rows[None, :], 1, 8, 0.5)[0]
    assert (got - ID_BASE).tolist() == rows[_select_one(_gathered(idx, rows), q, 1, 8, 0.5)].tolist()


def test_256_queries_in_one_launch_equal_their_own_launches():
    idx, _ = _small_index(n_rows=2000, seed=9)
    rng = np.random.default_rng(13)
    ids = ID_BASE + np.stack([rng.permutation(2000)[:20] for _ in range(256)])
    qs = rng.integers(-300, 300, (256, 64)) / 128.0
    for k in (5, 2):                                             # (k = 5: the pairs first; k = 2: round by round)
        out = _select_rows(idx, qs, ids, 1, k, 0.5)
        assert (out >= ID_BASE).all()
        for r in range(256):
            one = _select_rows(idx, qs[r: r + 1], ids[r: r + 1], 1, k, 0.5)[0]
            assert out[r].tolist() == one.tolist(), r
        for r in range(256):
            want = _select_one(_gathered(idx, ids[r] - ID_BASE), qs[r], 1, k, 0.5)
            assert out[r].tolist() == ids[r][want].tolist(), r


def test_engine_entry_point_chunks_under_its_workspace_cap():
    """FlatIndexF16.mmr_select_device: same answer whether the batch goes through in one launch or, with the cap lowered, in
    runs of three queries; the workspace is kept between calls; n beyond 1024 is refused."""
    import torch

    from rag_arc_amd.hip import binding as B

    idx, _ = _small_index(n_rows=1500, seed=21)
    rng = np.random.default_rng(14)
    ids = torch.from_numpy(ID_BASE + np.stack([rng.permutation(1500)[:33] for _ in range(10)])).cuda()
    ids[4, 20:] = -1
    qs = rng.standard_normal((10, 64))
    whole = idx.mmr_select_device(qs, ids, 7, 0.3).cpu().numpy()
    assert whole.shape == (10, 7) and (whole >= ID_BASE).all()
    ws = idx._mmr_ws
    assert idx.mmr_select_device(qs, ids, 7, 0.3).cpu().numpy().tolist() == whole.tolist() and idx._mmr_ws is ws
    idx.MMR_WS_CAP_BYTES = 3 * int(idx.lib.rarc_mmr_rows_workspace_bytes(1, 33, 64)) + 8
    assert idx.mmr_select_device(qs, ids, 7, 0.3).cpu().numpy().tolist() == whole.tolist()
    for r in (0, 4, 9):
        assert _select_rows(idx, qs[r: r + 1], ids[r: r + 1].cpu().numpy(), 0, 7, 0.3)[0].tolist() == whole[r].tolist()
    assert idx.mmr_select_device(qs, ids, 7, 0.3, normalize=True).cpu().numpy().tolist() == \
        _select_rows(idx, qs, ids.cpu().numpy(), 1, 7, 0.3).tolist()
    with pytest.raises(B.RarcUnsupported):
        idx.mmr_select_device(qs, torch.zeros((10, 1025), dtype=torch.int64, device="cuda"), 7)
