"""The knn_graph oracle (tests/knn_ref.py) pinned on the CPU: against scikit-learn's cosine_similarity — the function the
reference calls for its other self-join — plus a plain python top-K, against a brute-force double loop, and THE GUARD: on every
input of the GPU file's exact category the 1e-12 band excuses nothing (no cosine within the band of a row's K-th best or of the
cutoff, and every gap inside an answer far above float64 noise), so the comparison there is plain equality of ids in order."""
import math
import os

import numpy as np
import pytest

from tests import knn_ref as R

_FIRST, _LAST = (int(v) for v in os.environ.get("RARC_FUZZ_SEEDS", "0:10").split(":"))


def _python_topk(sim, top_k, cutoff):
    out = []
    for i in range(len(sim)):
        cand = [(-float(sim[i][j]), j) for j in range(len(sim)) if j != i and sim[i][j] >= cutoff]
        out.append([(j, -s) for s, j in sorted(cand)[:top_k]])
    return out


def _as_lists(got):
    ids, cos, cnt = got
    return [[(int(ids[i, t]), float(cos[i, t])) for t in range(cnt[i])] for i in range(len(cnt))]


@pytest.mark.parametrize("n,d,top_k,cutoff", [(40, 7, 3, 0.0), (120, 16, 10, -1.0), (64, 3, 5, 0.85), (9, 5, 20, 0.0)])
def test_oracle_is_sklearns_cosine_plus_a_plain_topk(n, d, top_k, cutoff):
    pairwise = pytest.importorskip("sklearn.metrics.pairwise")
    x = R.planted(n + d, n, d, noise=0.2)
    x[n // 2] = 0.0                                                   # a zero row: cosine 0 with everything
    sim = pairwise.cosine_similarity(np.asarray(x, dtype=np.float64))
    assert np.max(np.abs(sim - R.cosine_matrix_f64(x))) <= 1e-14
    got = R.knn_from_sim(sim, top_k, cutoff)
    assert _as_lists(got) == _python_topk(sim, top_k, cutoff)
    ids, cos, cnt = got
    assert np.all(ids[np.arange(top_k)[None, :] >= cnt[:, None]] == -1) and np.all(np.isneginf(cos[np.arange(top_k)[None, :] >= cnt[:, None]]))


def test_oracle_against_a_double_loop():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((12, 4))
    x[3] = 2.5 * x[7]                                                 # a scaled copy: cosine 1 up to rounding
    x[5] = 0.0
    want = []
    for i in range(12):
        row = []
        for j in range(12):
            if j == i:
                continue
            ni, nj = math.sqrt(sum(v * v for v in x[i])), math.sqrt(sum(v * v for v in x[j]))
            c = sum(a * b for a, b in zip(x[i] / (ni or 1.0), x[j] / (nj or 1.0)))
            if c >= 0.0:
                row.append((-c, j))
        want.append([j for _, j in sorted(row)[:4]])
    ids, cos, cnt = R.knn_graph_f64(x, 4, 0.0)
    assert [ids[i, :cnt[i]].tolist() for i in range(12)] == want
    assert ids[3, 0] == 7 and ids[7, 0] == 3 and abs(cos[3, 0] - 1.0) < 1e-15
    assert cnt[5] == 4 and ids[5].tolist() == [0, 1, 2, 3] and np.all(cos[5] == 0.0)      # zero row: ties at 0, by id
    e_ids, e_cos, e_cnt = R.knn_graph_f64(x[:1], 4, 0.0)
    assert e_ids.shape == (1, 4) and e_cnt.tolist() == [0] and np.all(e_ids == -1) and np.all(np.isneginf(e_cos))


def test_compare_rejects_wrong_answers():
    x = R.planted(3, 200, 16, noise=0.1)
    sim = R.cosine_matrix_f64(x)
    ids, cos, cnt = R.knn_from_sim(sim, 5, 0.0)
    R.compare((ids, cos, cnt), sim, 5, 0.0)
    for spoil in ("swap", "self", "score", "count", "missing"):
        i2, c2, n2 = ids.copy(), cos.copy(), cnt.copy()
        if spoil == "swap":
            i2[7, [0, 1]] = i2[7, [1, 0]]
        elif spoil == "self":
            i2[7, 2] = 7
        elif spoil == "score":
            c2[7, 2] += 1e-9
        elif spoil == "count":
            n2[7] -= 1
        else:
            worst = int(np.argmin(sim[7]))
            i2[7, 4], c2[7, 4] = worst, sim[7, worst]
        with pytest.raises(AssertionError):
            R.compare((i2, c2, n2), sim, 5, 0.0)


def _guard(case):
    seed, n, d, top_k, cutoff, noise = case
    sim = R.cosine_matrix_f64(R.exact_input(case))
    assert R.band_rows(sim, top_k, cutoff) == 0, case
    # ... and a band 1000 times as wide still excuses nothing: the seeds were not picked on a knife's edge
    assert R.band_rows(sim, top_k, cutoff, band=1e-9) == 0, case
    assert R.min_gap_in_answers(R.knn_from_sim(sim, top_k, cutoff)) > 1e-10, case


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: "n%d-d%d-k%d-c%g" % (c[1], c[2], c[3], c[4]))
def test_guard_exact_cases_have_nothing_in_the_band(case):
    _guard(case)


@pytest.mark.parametrize("seed", range(_FIRST, _LAST))
def test_guard_exact_sweep_has_nothing_in_the_band(seed):
    _guard(R.fuzz_case(seed))


def test_guard_threshold_inputs():
    x, (late, tail), (early, head) = R.threshold_input()
    sim = R.cosine_matrix_f64(x)
    ids, _, _ = R.knn_from_sim(sim, 10, -1.0)
    assert np.array_equal(ids[late, 0], tail) and np.array_equal(ids[early, 0], head)       # the planted row IS the nearest
    for cutoff in (-1.0, 0.85):
        assert R.band_rows(sim, 10, cutoff) == 0
        assert R.min_gap_in_answers(R.knn_from_sim(sim, 10, cutoff)) > 1e-10


def test_tie_inputs_are_ties():
    """The tie category's inputs do NOT pass the guard: that is what makes them the tie category."""
    assert R.band_rows(R.cosine_matrix_f64(R.scaled_copies()), 10, 0.85) > 500
    x, at = R.identical_copies()
    assert len(at) == 40 and all(np.array_equal(x[a], x[at[0]]) for a in at)
    assert R.band_rows(R.cosine_matrix_f64(R.one_dimension()), 10, 0.0) > 0


# ---- the long-list inputs of tests/test_gpu_self_join_lists.py -------------------------------------------------------------------

def test_long_pair_lists_is_the_smallest_input_with_256_columns_past_one_block():
    """The float64 cosine matrix itself shows 256 columns with more than 1024 + 64 true pairs (the nominees are a superset of
    them: a lower bound on the lists similar_pairs walks), one row fewer shows 255, and no cosine lies within 1e-9 of the
    threshold: the pair set is decided."""
    x = R.long_pair_lists()
    n, thr = R.LONG_PAIRS_N, R.LONG_PAIRS_THR
    assert x.shape == (n, 3) and x.dtype == np.float32
    sim = R.cosine_matrix_f64(x)
    per_column = np.triu(sim >= thr, 1).sum(axis=0)
    long_cols = np.nonzero(per_column > R.LONG_PAIRS_OVER)[0]
    assert len(long_cols) == 256 and long_cols[-1] == n - 1 and long_cols[0] > 2600
    assert np.abs(sim[np.triu_indices(n, 1)] - thr).min() > 1e-9
    pairs, cos = R.pairs_from_sim(sim, thr)
    assert len(pairs) == per_column.sum() > 1_700_000 and np.all(pairs[:, 0] < pairs[:, 1]) and np.all(cos >= thr)
    assert np.array_equal(np.bincount(pairs[:, 1], minlength=n), per_column)
    key = pairs[:, 0] * n + pairs[:, 1]
    assert np.all(key[1:] > key[:-1])                                                  # ordered by (i, j), as the reference's loop
    few = R.long_pair_lists(n=300)                                                     # pairs_from_sim is the oracle's double loop
    from oracle import cpu_ref
    p300, c300 = R.pairs_from_sim(R.cosine_matrix_f64(few), thr)
    assert cpu_ref.similar_pairs_f64(few, thr) == list(zip(p300[:, 0].tolist(), p300[:, 1].tolist(), c300.tolist()))
    led = R.long_pair_lists(lead=4097)                                                 # the same rows behind 4097 zero rows
    assert led.shape == (4097 + n, 3) and not led[:4097].any() and np.array_equal(led[4097:], x)


def _tight(which):
    seed, m = which
    x, at, marks = R.tight_cluster(seed, m, probe=R.TIGHT_PROBE if which == R.TIGHT_LARGE else 0.0)
    return x, at, marks, R.cosine_matrix_f64(x)


@pytest.mark.parametrize("which,top_k", [(w, k) for w in (R.TIGHT_SMALL, R.TIGHT_LARGE) for k in R.TIGHT_TOP_KS[w]],
                         ids=lambda v: "m%d" % v[1] if isinstance(v, tuple) else "k%d" % v)
def test_tight_cluster_keeps_every_list_long_and_every_answer_decided(which, top_k):
    """What the GPU file relies on, from the oracle alone.  (1) Every in-cluster cosine exceeds 1 - eps / 2: a cluster row's
    approximate score is then above 1 - 1.5 eps, and no threshold a_K - 2 eps can pass 1 - eps, so every cluster column's list
    holds all m cluster rows to the end.  (2) The band excuses nothing for any (top_k, cutoff) used, and consecutive cosines of
    every answer differ by more than 1e-14: a float64 cosine of 16 dimensions carries at most about a dozen roundings of
    1.1e-16, the kernel's and the oracle's together under 3e-15 per pair, so a gap above 1e-14 cannot close — the order of the
    ids is the oracle's.  (3) The cluster's indices reach into every chunk of rows."""
    x, at, marks, sim = _tight(which)
    m, n = which[1], which[1] + R.TIGHT_BACKGROUND
    assert x.shape == (n, R.TIGHT_D) and len(at) == m and np.all(np.diff(at) > 0)
    eps = R.pairs_eps(R.d_pad_of(R.TIGHT_D))
    inside = R.cluster_cosines(sim, at)
    assert inside.min() > 1.0 - eps / 2, 1.0 - inside.min()
    for lo, hi in ((0, 512), (512, 768), (768, 2560), (n - 256, n)):                  # the chunk edges of top_k 10 and 256
        assert np.count_nonzero((at >= lo) & (at < hi)) > (hi - lo) // 3
    norms = np.linalg.norm(x[at].astype(np.float64), axis=1)
    assert norms.min() < 0.3 and norms.max() > 4.0                                     # any scale: the kernel normalises
    cutoffs = R.tight_cutoffs(sim, at)
    assert cutoffs[:2] == (-1.0, 0.85) and inside.min() < cutoffs[2] < inside.max()
    in_cluster = np.zeros(n, bool)
    in_cluster[at] = True
    for cutoff in cutoffs:
        assert R.band_rows(sim, top_k, cutoff) == 0, (top_k, cutoff)
        want = R.knn_from_sim(sim, top_k, cutoff)
        assert R.min_gap_in_answers(want) > 1e-14, (top_k, cutoff)
        ids, _, cnt = want
        assert in_cluster[ids[at][ids[at] >= 0]].all()                                 # a cluster row's neighbours are cluster rows
        if cutoff < 0.9:
            assert np.all(cnt[at] == top_k)
        elif top_k == 256:                                                             # the median cutoff thins: counts differ by row
            assert 0 < np.count_nonzero(cnt[at] < top_k) < m and cnt[at].max() == top_k


def test_tight_cluster_probe_row_has_the_whole_cluster_near_its_best_neighbour():
    """The large input's probe column: its best neighbour's cosine is ~0.996, so with top_k = 1 its threshold settles 2 eps
    under that — and nearly the whole cluster lies above: a list past 4096 entries while the column's own score of 1 stands
    2 eps clear of every other.  (Expected, not proven: the count below leaves eps / 2 for the actual errors of the approximate
    scores, which are a few 1e-4; a library whose select counts the own row returns no neighbour for this column.)"""
    x, at, marks, sim = _tight(R.TIGHT_LARGE)
    p, eps = marks["probe"], R.pairs_eps(R.d_pad_of(R.TIGHT_D))
    assert p >= 0 and p not in at and abs(np.linalg.norm(x[p]) - 1.0) < 1e-6
    others = np.delete(sim[p], p)
    assert others.max() < 1.0 - 2.0 * eps - 1e-3
    assert np.count_nonzero(others >= others.max() - 1.5 * eps) > 4096 + 64


def test_thinned_input_has_a_zero_row_a_short_answer_and_rows_without_neighbours():
    seed, m = R.TIGHT_SMALL
    x, at, marks = R.tight_cluster(seed, m, zero_rows=1, group=4)
    plain = R.tight_cluster(seed, m)[0]
    changed = np.nonzero((x != plain).any(axis=1))[0]
    assert set(changed) == set(marks["zeroed"]) | set(marks["group"][1:]) and marks["probe"] == -1
    sim = R.cosine_matrix_f64(x)
    assert R.band_rows(sim, 10, 0.85) == 0
    ids, cos, cnt = R.knn_from_sim(sim, 10, 0.85)
    assert R.min_gap_in_answers((ids, cos, cnt)) > 1e-14
    assert not x[marks["zeroed"]].any() and np.all(cnt[marks["zeroed"]] == 0) and not np.isin(ids, marks["zeroed"]).any()
    assert len(marks["group"]) == 5 and np.all(cnt[marks["group"]] == 4)             # fewer than top_k survivors
    assert np.all(cnt[at] == 10) and np.count_nonzero(cnt == 0) > 600                 # most background rows: no neighbour at all


def test_many_identical_copies_are_bit_identical_and_fill_more_than_a_buffer():
    x, at = R.many_identical_copies()
    assert x.shape == (1500, 8) and len(at) == 1300 > 1024 + 64 and np.all(np.diff(at) > 0)
    assert all(np.array_equal(x[a], x[at[0]]) for a in at)
    rest = np.setdiff1d(np.arange(1500), at)
    assert not any(np.array_equal(x[r], x[at[0]]) for r in rest)
