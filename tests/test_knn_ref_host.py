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
