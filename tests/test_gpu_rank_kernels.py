"""The rank-level kernels at their limits: rarc_rrf_fuse, rarc_rerank_order, rarc_mmr_select (csrc/fuse.hip), rarc_topk_merge,
rarc_topk_merge_packed and rarc_pack_results (csrc/finalize.hip), each against the plain restatements of tests/rank_ref.py
(held to the recorded goldens and the oracle by tests/test_rank_ref_host.py), at the sizes where their loops take a second,
a last and a padding trip, on both sides of every declared limit, and through the bindings the product uses.

Declared limits and where they are met:  RRF 4096 items (4096 accepted, 4097 refused) and 64 lists (64 / 65);  rerank 4096
(4096 / 4097);  merge: G k <= 8192 after rounding up to a power of two — the 160 KiB LDS gate — ((8, 1024), (5, 1638), (64, 128)
accepted, (8, 1025) refused);  MMR 1024 candidates (1024 / 1025), ld >= d, k >= 1.
"""
import numpy as np
import pytest

from tests import rank_ref as R

pytestmark = pytest.mark.gpu


def _lib():
    from rag_arc_amd.hip import binding as B

    return B, B.load_library()


# ===================================================================================================================== RRF
RRF_TOTALS = (255, 256, 257, 1023, 1024, 1025, 4095, 4096)
RRF_SHAPES = {"2x2048": (2, 2048, False), "64x64": (64, 64, False), "64ragged": (64, 64, True), "1x4096": (1, 4096, False)}
RRF_KS = (60.0, 0.5, 2.0 ** -10, 1.0, 1000.0)


@pytest.mark.parametrize("total", RRF_TOTALS)
@pytest.mark.parametrize("shape", list(RRF_SHAPES))
def test_rrf_at_every_trip_boundary(oracle, total, shape):
    """6 queries per launch (even ones hold exactly `total` items, odd ones some other number, so neighbouring blocks differ),
    every key population, rrf_k from 2^-10 to 1000, top_k of 0, 1, fewer than / exactly / more than the distinct count:
    fused keys, fp64 scores (==, never approx) and counts equal oracle.rrf_fuse; slots past the count keep fuse_ids' fill."""
    import torch

    from rag_arc_amd.core.utils import HipRRFusion

    n_lists, max_len, ragged = RRF_SHAPES[shape]
    nq = 6
    for pi, pop in enumerate(R.RRF_POPULATIONS):
        rng = np.random.default_rng([total, n_lists, max_len, int(ragged), pi])
        keys = R.rrf_keys(rng, nq, n_lists, max_len, pop)
        lens = R.rrf_lens(rng, nq, n_lists, max_len, total, ragged)
        assert lens[0].sum() == total
        rrf_k = RRF_KS[pi]
        full = R.rrf_rows(oracle, keys, lens, rrf_k, n_lists * max_len + 8)
        distinct0 = len(full[0][0])
        d_keys, d_lens = torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda()
        for top_k in sorted({0, 1, max(1, distinct0 // 2), distinct0, distinct0 + 7}):
            fk, fs, fn = HipRRFusion(k=rrf_k).fuse_ids(d_keys, d_lens, top_k)
            fk, fs, fn = fk.cpu().numpy(), fs.cpu().numpy(), fn.cpu().numpy()
            assert fk.shape == (nq, top_k) and fs.shape == (nq, top_k)
            for b in range(nq):
                what = f"seed=({total},{n_lists},{max_len},{int(ragged)},{pi}) pop={pop} rrf_k={rrf_k} top_k={top_k} query={b} items={lens[b].sum()}"
                wk, ws = full[b][0][:top_k], full[b][1][:top_k]
                assert fn[b] == len(wk), what
                assert fk[b, : fn[b]].tolist() == wk, what
                assert fs[b, : fn[b]].tolist() == ws, what                        # python float ==: exact fp64
                assert (fk[b, fn[b]:] == -1).all() and (fs[b, fn[b]:] == 0.0).all(), what


def test_rrf_one_key_in_every_one_of_64_lists(oracle):
    """The fp64 sum whose ORDER is the point: a key present in all 64 lists (a 64-link chain), at every position class."""
    import torch

    from rag_arc_amd.core.utils import HipRRFusion

    rng = np.random.default_rng(64)
    keys = R.rrf_keys(rng, 8, 64, 64, "everywhere")
    lens = np.full((8, 64), 64, np.int32)
    for rrf_k in (60.0, 0.1):
        fk, fs, fn = HipRRFusion(k=rrf_k).fuse_ids(torch.from_numpy(keys).cuda(), torch.from_numpy(lens).cuda(), 50)
        for b, (wk, ws) in enumerate(R.rrf_rows(oracle, keys, lens, rrf_k, 50)):
            assert fk[b].tolist() == wk and fs[b].tolist() == ws and int(fn[b]) == 50
            assert wk[0] == 777_777_777                                           # 64 terms beat everything else


def test_rrf_refusals_write_nothing():
    import torch

    from rag_arc_amd.core.utils import HipRRFusion, RetrievalResult, Document

    B, lib = _lib()
    for n_lists, max_len, code in ((1, 4097, -4), (17, 241, -4), (65, 1, -1), (65, 63, -1)):
        assert n_lists * max_len == 4097 or n_lists == 65
        keys = torch.ones((2, n_lists, max_len), dtype=torch.int64, device="cuda")
        lens = torch.ones((2, n_lists), dtype=torch.int32, device="cuda")
        ok, os_, on = (torch.full((2, 5), -9, dtype=torch.int64, device="cuda"), torch.full((2, 5), -9.0, dtype=torch.float64, device="cuda"),
                       torch.full((2,), -9, dtype=torch.int32, device="cuda"))
        rc = lib.rarc_rrf_fuse(keys.data_ptr(), lens.data_ptr(), 2, n_lists, max_len, 60.0, 5, ok.data_ptr(), os_.data_ptr(), on.data_ptr(), 0)
        assert rc == code
        with pytest.raises(B.RarcError, match=rf"\({code}\)"):
            B.check(rc, "rarc_rrf_fuse")
        torch.cuda.synchronize()
        assert (ok == -9).all() and (os_ == -9.0).all() and (on == -9).all()
        with pytest.raises(B.RarcError, match=rf"rarc_rrf_fuse failed \({code}\)"):
            HipRRFusion().fuse_ids(keys, lens, 5)
    # the FusionMethod forms raise too (they never hand back unfilled tensors)
    def results(n_lists, n):
        return [[RetrievalResult(document=Document(content=f"l{li}p{i}"), score=1.0) for i in range(n)] for li in range(n_lists)]

    for n_lists, n in ((65, 2), (2, 2049)):
        with pytest.raises(B.RarcError, match="rarc_rrf_fuse failed"):
            HipRRFusion().fuse(results(n_lists, n), 10)
        with pytest.raises(B.RarcError, match="rarc_rrf_fuse failed"):
            HipRRFusion().fuse_many([results(2, 3), results(n_lists, n)], 10)
    assert len(HipRRFusion().fuse(results(64, 64), 4096)) == 4096               # the limit itself is served


# ================================================================================================================== rerank
@pytest.mark.parametrize("n", R.RERANK_NS)
def test_rerank_order_is_total_at_every_size(oracle, n):
    """Nine rows per n (rank_ref.rerank_rows): the permutation is read back and judged on the host before anything indexes
    with it — exactly oracle.stable_desc_order of the kernel's own scores, a permutation of range(n), NaN last."""
    from rag_arc_amd.core.rerank import HipLogitReranker

    zn, zy, finite = R.rerank_rows(n)
    scores, perm = HipLogitReranker(lambda q, texts: (None, None)).score_order(zn, zy)
    scores, perm = scores.cpu().numpy(), perm.cpu().numpy()
    with np.errstate(all="ignore"):
        want = oracle.rerank_scores_f16(zn, zy)
    for b in range(zn.shape[0]):
        assert R.is_permutation(perm[b], n), f"n={n} row={b}: not a permutation of range(n)"
        assert perm[b].tolist() == R.rerank_order(oracle, scores[b]).tolist(), f"n={n} row={b}"
        nan_w = np.isnan(want[b].astype(np.float32))
        assert np.isnan(scores[b].astype(np.float32))[nan_w].all(), f"n={n} row={b}: a NaN of the oracle is a number here"
        if nan_w.any():                                                           # NaN last, in input order
            assert perm[b][n - int(np.isnan(scores[b].astype(np.float32)).sum()):].tolist() == \
                np.flatnonzero(np.isnan(scores[b].astype(np.float32))).tolist()
    got, ref = scores[finite].astype(np.float64), want[finite].astype(np.float64)
    tol = np.maximum(np.abs(ref) * 2.0 ** -6, 2.0 ** -24)                         # exp amplifies a last-place ls flip
    frac = float((scores[finite] == want[finite]).mean())
    print(f"rerank n={n}: max |delta| / tol = {np.max(np.abs(got - ref) / tol):.3f}, bit-equal {frac:.5f}")
    assert np.all(np.abs(got - ref) <= tol)
    assert frac > 0.98


def test_rerank_refuses_4097_and_raises():
    import torch

    from rag_arc_amd.core.rerank import HipLogitReranker

    B, lib = _lib()
    z = torch.zeros((1, 4097), dtype=torch.float16, device="cuda")
    sc = torch.full((1, 4097), 7.0, dtype=torch.float16, device="cuda")
    pm = torch.full((1, 4097), -9, dtype=torch.int32, device="cuda")
    assert lib.rarc_rerank_order(z.data_ptr(), z.data_ptr(), 1, 4097, sc.data_ptr(), pm.data_ptr(), 0) == -4
    torch.cuda.synchronize()
    assert (pm == -9).all() and (sc == 7.0).all()
    with pytest.raises(B.RarcError, match=r"rarc_rerank_order failed \(-4\)"):
        HipLogitReranker(lambda q, t: (None, None)).score_order(np.zeros((1, 4097), np.float16), np.zeros((1, 4097), np.float16))


def test_rerank_with_logits_beyond_fp16_keeps_every_document(oracle):
    """fp32 logits above 65504 become (inf, inf) in fp16 and p_yes NaN: those documents go last, in retrieval order; the
    others are ordered as ever; every returned object is one of the inputs."""
    from rag_arc_amd.core.rerank import HipLogitReranker
    from rag_arc_amd.core.utils import Document

    rng = np.random.default_rng(12)
    n = 300
    docs = [Document(content=f"d{i}") for i in range(n)]
    zn, zy = (rng.standard_normal(n) * 3).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)
    zn[[41, 7]], zy[[41, 7]] = (1.0e5, 7.0e4), (9.0e4, 2.0e5)
    table = {f"d{i}": (zn[i], zy[i]) for i in range(n)}
    rr = HipLogitReranker(lambda q, texts: ([table[t][0] for t in texts], [table[t][1] for t in texts]))
    out = rr.rerank("q", docs)
    assert len(out) == n and len({id(o) for o in out}) == n and all(o is docs[int(o.content[1:])] for o in out)
    assert [o.content for o in out[-2:]] == ["d7", "d41"]                          # retrieval order, not the order of the logits
    scores, perm = rr.score_order(zn, zy)                                           # the same cast to fp16, read back this time
    scores, perm = scores.cpu().numpy()[0], perm.cpu().numpy()[0]
    assert np.flatnonzero(np.isnan(scores.astype(np.float32))).tolist() == [7, 41]
    assert perm.tolist() == R.rerank_order(oracle, scores).tolist() and [int(o.content[1:]) for o in out] == perm.tolist()
    rest = [i for i in range(n) if i not in (7, 41)]
    want = oracle.rerank_scores_f16(zn[rest].astype(np.float16), zy[rest].astype(np.float16)).astype(np.float64)
    assert np.all(np.abs(scores[rest].astype(np.float64) - want) <= np.maximum(np.abs(want) * 2.0 ** -6, 2.0 ** -24))
    assert [o.content for o in rr.rerank("q", docs, k=5)] == [f"d{i}" for i in perm[:5]]


# =================================================================================================================== merge
MERGE_SHAPES = [(1, 1), (1, 100), (2, 1), (3, 7), (8, 1024), (5, 1638), (64, 128)]


def _merge_both_forms(torch, ids, sc, k):
    from rag_arc_amd.hip.sharded import ShardedFlatSearch, pack_results

    B, lib = _lib()
    G, nq, _ = ids.shape
    s = ShardedFlatSearch.__new__(ShardedFlatSearch)
    s.torch = torch
    d_ids, d_sc = torch.from_numpy(ids).cuda(), torch.from_numpy(sc).cuda()
    mi, ms = s._hip_merge(d_ids, d_sc, k)
    packed = torch.full((G, nq, k, 3), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for g in range(G):
        B.check(lib.rarc_pack_results(d_ids[g].data_ptr(), d_sc[g].data_ptr(), nq, k, packed[g].data_ptr(), 0), "rarc_pack_results")
    assert torch.equal(packed, pack_results(torch, d_ids, d_sc))                  # bit for bit, id -1 and the high words included
    pi = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    ps = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    B.check(lib.rarc_topk_merge_packed(packed.data_ptr(), G, nq, k, pi.data_ptr(), ps.data_ptr(), 0), "rarc_topk_merge_packed")
    return (mi.cpu().numpy(), ms.cpu().numpy()), (pi.cpu().numpy(), ps.cpu().numpy())


@pytest.mark.parametrize("G,k", MERGE_SHAPES)
def test_merge_at_every_shape(oracle, G, k):
    """ids over [0, 2^63) (the packed high word carries half the id), scores from a handful of levels (ids decide), +-0.0,
    short shards, a query with nothing, a query with fewer than k entries: ids and score BITS equal the comparator sort, in
    the plain and in the packed form."""
    import torch

    nq = 5 if G * k > 2048 else 12
    rng = np.random.default_rng([G, k, 5])
    ids, sc = R.merge_inputs(rng, G, nq, k)
    if (ids >= 0).sum() > 8:
        assert (ids[ids >= 0] >> 32).max() > 0
    wi, ws = R.merge(ids, sc, k)
    oi, os_ = oracle.topk_merge(ids, sc, k)
    assert np.array_equal(wi, oi) and np.array_equal(ws.view(np.uint32), os_.view(np.uint32))     # signed zeros included
    assert (wi[0] == -1).all() and np.isneginf(ws[0]).all()
    for form, (gi, gs) in zip(("plain", "packed"), _merge_both_forms(torch, ids, sc, k)):
        for q in range(nq):
            assert gi[q].tolist() == wi[q].tolist(), f"{form} G={G} k={k} seed=({G},{k},5) query={q}: ids"
            assert gs[q].view(np.uint32).tolist() == ws[q].view(np.uint32).tolist(), f"{form} G={G} k={k} query={q}: score bits"


def test_merge_refuses_what_the_lds_gate_excludes():
    import torch

    from rag_arc_amd.hip.sharded import ShardedFlatSearch

    B, lib = _lib()
    s = ShardedFlatSearch.__new__(ShardedFlatSearch)
    s.torch = torch
    for G, k in ((8, 1025), (1, 8193), (65, 128)):
        ids = torch.zeros((G, 2, k), dtype=torch.int64, device="cuda")
        sc = torch.zeros((G, 2, k), dtype=torch.float32, device="cuda")
        oi = torch.full((2, k), -9, dtype=torch.int64, device="cuda")
        os_ = torch.full((2, k), -9.0, dtype=torch.float32, device="cuda")
        assert lib.rarc_topk_merge(ids.data_ptr(), sc.data_ptr(), G, 2, k, oi.data_ptr(), os_.data_ptr(), 0) == -4
        packed = torch.zeros((G, 2, k, 3), dtype=torch.int32, device="cuda")
        assert lib.rarc_topk_merge_packed(packed.data_ptr(), G, 2, k, oi.data_ptr(), os_.data_ptr(), 0) == -4
        torch.cuda.synchronize()
        assert (oi == -9).all() and (os_ == -9.0).all()
        with pytest.raises(B.RarcError, match=r"rarc_topk_merge failed \(-4\)"):
            s._hip_merge(ids, sc, k)
    with pytest.raises(ValueError):
        s._hip_merge(torch.zeros((2, 2, 8), dtype=torch.int64, device="cuda"), torch.zeros((2, 2, 8), device="cuda"), 4)


def test_signed_zero_merge_equals_search_of_the_whole(oracle):
    """What a single-shard search does with +0.0 and -0.0, and that the merge of shards does the same.  fp32 rows, raw inner
    product: row 1's products all underflow to -0 (or are -0), so its canonical score is -0.0; rows 0 and 2 score +0.0.  A
    search sorts by rarc_candkey, the sign-magnitude bit pattern: +0.0 ahead of -0.0 whatever the row numbers."""
    import torch

    from rag_arc_amd.hip.engine import FlatIndexF16
    from rag_arc_amd.hip.sharded import ShardedFlatSearch

    d, k = 128, 6
    X = np.zeros((6, d), np.float32)
    for r in (1, 4):
        X[r] = -0.0
        X[r, :8] = -1e-30                       # 1e-30 * -1e-30 rounds to -0.0 in every one of the eight chains
    X[3, 8], X[5, 8] = 1.0, 0.5                 # (column 8 is -0.0 in rows 1 and 4: the product with q[8] = 1 is -0.0 too)
    q = np.zeros((1, d), np.float32)
    q[0, :8], q[0, 8] = 1e-30, 1.0
    rows = oracle.ingest_f32(X, normalize=False)[0]
    oi, osc = oracle.flat_search_f32(rows, q, k)[:2]
    assert oi.tolist() == [[3, 5, 0, 2, 1, 4]] and np.signbit(osc).tolist() == [[False, False, False, False, True, True]]
    whole = FlatIndexF16(d, metric="ip", storage="f32")
    whole.add(X)
    S, I = whole.search(q, k)
    print("single-shard search:", I.tolist(), S.tolist(), np.signbit(S).tolist())
    assert np.array_equal(I, oi) and np.array_equal(S.view(np.uint32), osc.view(np.uint32))
    # orthogonal fp16 rows with a sign flip: every product is a zero, the sum is +0.0 for both, the row number decides
    Y = np.zeros((3, d), np.float32)
    Y[0, 1], Y[1, 1], Y[2, 0] = 1.0, -1.0, -1.0
    q2 = np.zeros((1, d), np.float32)
    q2[0, 0] = 1.0
    flip = FlatIndexF16(d, metric="ip")
    flip.add(Y)
    S2, I2 = flip.search(q2, 3)
    oi2, os2, _ = oracle.flat_search_f16(oracle.ingest_f16(Y, normalize=False)[0], q2, 3)
    assert np.array_equal(I2, oi2) and np.array_equal(S2.view(np.uint32), os2.view(np.uint32)) and I2.tolist() == [[0, 1, 2]]
    # shards of the first corpus (each holds a row of ordinary size), merged on the device in both forms == the whole:
    # ids 0, 2 (+0.0) ahead of 1, 4 (-0.0), where "id ascending among equal scores" would say 0, 1, 2, 4
    split = (0, 4, 6)
    pi = np.full((len(split) - 1, 1, k), -1, np.int64)
    ps = np.full((len(split) - 1, 1, k), -np.inf, np.float32)
    for g, (a, b) in enumerate(zip(split[:-1], split[1:])):
        shard = FlatIndexF16(d, metric="ip", storage="f32", id_base=a)
        shard.add(X[a:b])
        s_, i_ = shard.search(q, k)
        pi[g], ps[g] = i_, s_
    assert pi[0, 0, :4].tolist() == [3, 0, 2, 1] and pi[1, 0, :2].tolist() == [5, 4]
    for form, (gi, gs) in zip(("plain", "packed"), _merge_both_forms(torch, pi, ps, k)):
        assert np.array_equal(gi, I) and np.array_equal(gs.view(np.uint32), S.view(np.uint32)), form
    for fn in (oracle.topk_merge, R.merge):
        mi, ms = fn(pi, ps, k)
        assert np.array_equal(mi, I) and np.array_equal(ms.view(np.uint32), S.view(np.uint32)), fn.__name__


# ===================================================================================================================== MMR
def _mmr_run(torch, B, lib, cand, q, normalize, k, lam, pad):
    """rarc_mmr_select over cand with row stride d + pad (the padding filled with 1e30, which must not leak in): the k outputs,
    the buffer pre-filled with -7."""
    n, d = cand.shape
    wide = np.full((n, d + pad), 1.0e30, np.float32)
    wide[:, :d] = cand
    d_c, d_q = torch.from_numpy(wide).cuda(), torch.from_numpy(q).cuda()
    work = torch.empty(int(lib.rarc_mmr_workspace_doubles(n, d)), dtype=torch.float64, device="cuda")
    out = torch.full((k,), -7, dtype=torch.int32, device="cuda")
    B.check(lib.rarc_mmr_select(d_c.data_ptr(), d + pad, d_q.data_ptr(), n, d, normalize, k, float(lam), work.data_ptr(), out.data_ptr(), 0),
            "rarc_mmr_select")
    return out.cpu().numpy()


@pytest.mark.parametrize("n", R.MMR_NS)
@pytest.mark.parametrize("d", R.MMR_DS)
def test_mmr_picks_lie_in_the_near_best_set(n, d):
    """Every lambda x normalize, without and with built ties (rank_ref.mmr_cases), k = n + 3 (the first n outputs are defined)
    with the row stride alternating between d and d + 5; the kernel's own picks are walked through the longdouble reference:
    each within mmr_tol of the best, equal to it where it stands alone, the lowest index among exactly equal candidates.
    The greedy selection for a smaller k is a prefix: k = 1, 2 and n are run with the other stride and compared with it."""
    import torch

    B, lib = _lib()
    for ci, (lam, nm, ties, seed) in enumerate(R.mmr_cases(n, d)):
        what = f"n={n} d={d} lam={lam} normalize={nm} ties={ties} seed={seed}"
        cand, q = R.mmr_inputs(n, d, seed, ties)
        pad = 5 if ci % 2 == 0 else 0
        out = _mmr_run(torch, B, lib, cand, q, nm, n + 3, lam, pad)
        picks = out[:n].tolist()
        assert R.is_permutation(picks, n), what
        ref = R.MMRRef(cand, q, nm, lam)
        wide = R.mmr_check_walk(ref, picks, what)
        if not R.mmr_ties_built(n, d, ties):
            assert wide <= 0.05 * max(n - 1, 1), (what, wide)
        for k in sorted({1, 2, n}):
            short = _mmr_run(torch, B, lib, cand, q, nm, k, lam, 5 - pad)
            assert short[: min(k, n)].tolist() == picks[: min(k, n)], (what, k)
            assert (short[min(k, n):] == -7).all(), (what, k)


def test_mmr_zero_vector_under_normalize_goes_last():
    """A zero candidate has no direction: normalised it is NaN and so is its value, which never compares above anything.  The
    kernel owes n valid picks all the same: the comparable candidates in MMR order, then the others by index."""
    import torch

    B, lib = _lib()
    n, d = 300, 64
    cand, q = R.mmr_inputs(n, d, 5, False)
    zeros = [3, 77, 256, 299]
    cand[zeros] = 0.0
    out = _mmr_run(torch, B, lib, cand, q, 1, n, 0.5, 0)
    picks = out.tolist()
    assert R.is_permutation(picks, n) and picks[-len(zeros):] == zeros
    keep = [i for i in range(n) if i not in zeros]
    ref = R.MMRRef(cand[keep], q, 1, 0.5)
    R.mmr_check_walk(ref, [keep.index(p) for p in picks[: len(keep)]], "zero rows removed")


def test_mmr_refusals():
    import torch

    B, lib = _lib()
    cand = torch.zeros((1025, 8), dtype=torch.float32, device="cuda")
    q = torch.zeros(8, dtype=torch.float64, device="cuda")
    work = torch.zeros(1025 * 8 + 8, dtype=torch.float64, device="cuda")
    out = torch.full((16,), -7, dtype=torch.int32, device="cuda")
    for n, d, ld, k in ((1025, 8, 8, 4), (16, 8, 7, 4), (16, 8, 8, 0), (0, 8, 8, 4)):
        rc = lib.rarc_mmr_select(cand.data_ptr(), ld, q.data_ptr(), n, d, 0, k, 0.5, work.data_ptr(), out.data_ptr(), 0)
        assert rc == -1, (n, d, ld, k)
        with pytest.raises(B.RarcError, match="bad sizes"):
            B.check(rc, "rarc_mmr_select")
    torch.cuda.synchronize()
    assert (out == -7).all()
