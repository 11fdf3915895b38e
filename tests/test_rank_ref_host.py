"""tests/rank_ref.py against what the repository already pins (no GPU): the recorded RRF and MMR goldens, oracle.topk_merge,
and the conditions on INPUTS that tests/test_gpu_rank_kernels.py relies on (the MMR tie cap, the rerank bit-equality floor)."""
import numpy as np
import pytest

from oracle import cpu_ref as oracle
from tests import rank_ref as R
from tests.helpers import golden, unhex


def test_rrf_rows_reproduce_the_recorded_goldens():
    for case in golden("rrf.json"):
        contents = [[c for c in one] for one in case["lists"]]
        names = {}
        keys = [[names.setdefault(c if isinstance(c, str) else c["content"], len(names)) for c in one] for one in contents]
        n_lists, max_len = len(keys), max((len(one) for one in keys), default=0)
        if n_lists == 0 or max_len == 0:
            continue
        table = np.zeros((1, n_lists, max_len), np.int64)
        lens = np.zeros((1, n_lists), np.int32)
        for r, one in enumerate(keys):
            table[0, r, : len(one)], lens[0, r] = one, len(one)
        (fk, fs), = R.rrf_rows(oracle, table, lens, case["k"], case["top_k"])
        back = {v: k for k, v in names.items()}
        assert [back[k] for k in fk] == [g["content"] for g in case["fused"]]
        assert fs == [unhex(g["score_hex"]) for g in case["fused"]]


def test_rrf_generators_reach_the_sizes_they_promise():
    rng = np.random.default_rng(5)
    for n_lists, max_len, total, ragged in ((2, 2048, 4096, False), (64, 64, 4095, True), (64, 64, 257, True), (1, 4096, 1025, False),
                                            (64, 64, 4096, True), (2, 2048, 255, True)):
        lens = R.rrf_lens(rng, 6, n_lists, max_len, total, ragged)
        assert lens.min() >= 0 and lens.max() <= max_len
        assert lens[0].sum() == total and lens[2].sum() == total and lens[4].sum() == total
        if ragged and n_lists == 64 and total < 4096:
            assert (lens == 0).any()
    for pop in R.RRF_POPULATIONS:
        keys = R.rrf_keys(rng, 2, 64, 64, pop)
        assert keys.shape == (2, 64, 64) and keys.dtype == np.int64
    assert all((R.rrf_keys(rng, 1, 64, 64, "everywhere")[0] == 777_777_777).sum(axis=1) >= 1)
    wide = R.rrf_keys(rng, 1, 2, 2048, "wide")
    assert (wide == 0).any() and (wide < 0).any() and (wide >= 2 ** 32).any()


@pytest.mark.parametrize("G,nq,k", [(1, 4, 1), (3, 5, 7), (8, 6, 100), (5, 3, 333)])
def test_merge_equals_the_oracle_without_signed_zeros(G, nq, k):
    rng = np.random.default_rng([G, nq, k])
    ids, sc = R.merge_inputs(rng, G, nq, k)
    sc[sc == 0] = np.float32(0.5)                                  # no +-0 (the two zeros are the next test)
    wi, ws = oracle.topk_merge(ids, sc, k)
    ri, rs = R.merge(ids, sc, k)
    assert np.array_equal(ri, wi) and np.array_equal(rs.view(np.uint32), ws.view(np.uint32))
    assert (ri[0] == -1).all() and np.isneginf(rs[0]).all()        # query 0: every shard empty
    if nq > 1 and G * k > 1:
        assert 0 < (ri[1] >= 0).sum() < k or k == 1                # query 1: fewer than k entries in total


def test_merge_orders_plus_zero_above_minus_zero_like_a_search():
    """The rule of rarc_oracle.c's candkey (what every search sorts by): of +0.0 and -0.0 the positive one is ahead, whatever
    the ids; oracle.topk_merge and the restatement both follow it, and equal the oracle's own search of the whole."""
    ids = np.array([[[7, 9]], [[3, 5]]], np.int64)
    sc = np.array([[[0.0, -0.0]], [[0.0, -0.0]]], np.float32)
    for fn in (oracle.topk_merge, R.merge):
        mi, ms = fn(ids, sc, 4)
        assert mi.tolist() == [[3, 7, 5, 9]]
        assert np.signbit(ms).tolist() == [[False, False, True, True]]
    # a whole-corpus search that produces both zeros: every product of row 1 underflows to -0 (or is -0), row 0 / 2 give +0
    d = 128
    X = np.zeros((4, d), np.float32)
    X[1] = -0.0
    X[1, :8] = -1e-30
    X[3, 0] = 1.0
    q = np.zeros((1, d), np.float32)
    q[0, :8] = 1e-30
    rows = oracle.ingest_f32(X, normalize=False)[0]
    I, S = oracle.flat_search_f32(rows, q, 4)[:2]
    assert I.tolist() == [[3, 0, 2, 1]] and np.signbit(S).tolist() == [[False, False, False, True]]
    for split in ((0, 2, 4), (0, 1, 4), (0, 3, 4)):
        parts = [oracle.flat_search_f32(rows[a:b], q, 4, id_base=a)[:2] for a, b in zip(split[:-1], split[1:])]
        pi = np.full((len(parts), 1, 4), -1, np.int64)
        ps = np.full((len(parts), 1, 4), -np.inf, np.float32)
        for g, (i_, s_) in enumerate(parts):
            pi[g], ps[g] = i_, s_
        for fn in (oracle.topk_merge, R.merge):
            mi, ms = fn(pi, ps, 4)
            assert np.array_equal(mi, I) and np.array_equal(ms.view(np.uint32), S.view(np.uint32)), (split, fn.__name__)


def test_mmr_reference_follows_the_recorded_picks():
    for c in golden("mmr.json")["cases"]:
        E = np.array([[unhex(v) for v in row] for row in c["emb_hex"]], np.float64)
        q = np.array([unhex(v) for v in c["query_hex"]], np.float64)
        if c["k"] >= c["n"]:
            assert c["picked"] == list(range(c["n"]))               # _mmr_select returns the pool untouched
            continue
        if not np.array_equal(E.astype(np.float32).astype(np.float64), E):
            continue                                                # (MMRRef restates the kernel: fp32 candidates)
        ref = R.MMRRef(E, q, 0, c["lambda"])
        R.mmr_check_walk(ref, c["picked"], (c["n"], c["k"], c["lambda"]))


def test_mmr_reference_on_a_case_small_enough_to_do_by_hand():
    E = np.array([[1, 0], [1, 0], [0, 1], [0.5, 0.5]], np.float32)
    q = np.array([1.0, 0.25])
    ref = R.MMRRef(E, q, 0, 0.5)
    best, near, val = ref.step()                 # values: dup of 0: .5 - .5 = 0;  e2: .125 - 0;  e3: .3125 - .25 = .0625
    assert [float(v) for v in val[1:]] == [0.0, 0.125, 0.0625] and near.tolist() == [2] and float(best) == 0.125
    assert ref.tol == R.mmr_tol(2, ref.nu_q, ref.nu_c, 0, 0.5) and ref.nu_c == 1.0 and 12 * R.U < ref.tol < 13 * R.U
    with pytest.raises(AssertionError):
        R.mmr_check_walk(R.MMRRef(E, q, 0, 0.5), [0, 3, 2], "wrong on purpose")
    assert R.mmr_check_walk(R.MMRRef(E, q, 0, 0.5), [0, 2, 3, 1], "right") == 0


@pytest.mark.parametrize("n", R.MMR_NS)
@pytest.mark.parametrize("d", R.MMR_DS)
def test_mmr_inputs_stay_within_the_tie_cap(n, d):
    """The reference alone, choosing the lowest index of its own near-best set: at most 5 % of the steps of a case without
    built ties may offer more than one near-best candidate; and the redundancy term is active (never clamped at 0)."""
    for lam, nm, ties, seed in R.mmr_cases(n, d):
        cand, q = R.mmr_inputs(n, d, seed, ties)
        ref = R.MMRRef(cand, q, nm, lam)
        assert ref.gram.min() > 0
        wide = 0
        for _ in range(1, n):
            _, near, _ = ref.step()
            wide += near.size > 1
            ref.take(int(near[0]))
        if not R.mmr_ties_built(n, d, ties):
            assert wide <= 0.05 * max(n - 1, 1), (n, d, lam, nm, wide)
        elif n > 3 and lam < 1.0:
            assert wide >= 1                                        # the built ties are there


def test_rerank_inputs_meet_the_bit_equality_floor():
    """More than 98 % of the oracle's fp16 scores equal the same formula evaluated in float64 (rank_ref.p_yes_f64: the two
    fp16 tensors where the reference has them), for the finite rows the GPU test uses: the fraction it demands of the kernel is a property of the inputs, not a tuned number."""
    for n in R.RERANK_NS:
        zn, zy, finite = R.rerank_rows(n)
        if n >= 255:
            assert np.isnan(oracle.rerank_scores_f16(zn[~finite], zy[~finite]).astype(np.float32)).any(axis=1).all()
        want = oracle.rerank_scores_f16(zn[finite], zy[finite])
        exact = R.p_yes_f64(zn[finite], zy[finite])
        assert not np.isnan(want.astype(np.float32)).any()
        tol = np.maximum(np.abs(exact.astype(np.float64)) * 2.0 ** -6, 2.0 ** -24)
        assert np.all(np.abs(want.astype(np.float64) - exact.astype(np.float64)) <= tol)
        assert (want == exact).mean() > 0.98, (n, (want == exact).mean())
        for row in want:
            assert R.is_permutation(R.rerank_order(oracle, row), n)
    s = np.array([0.5, np.nan, 0.75, np.nan, 0.5, 0.0], np.float16)
    assert R.rerank_order(oracle, s).tolist() == [2, 0, 4, 5, 1, 3]      # NaN last, in input order
    assert not R.is_permutation([0, 0, 2], 3) and not R.is_permutation([0, 1], 3) and R.is_permutation([2, 0, 1], 3)
