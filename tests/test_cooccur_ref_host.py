"""tests/cooccur_ref.py, the yardstick of the co-occurrence tests, checked on its own: against the upper triangle of AᵀA where scipy
is installed, under permuted and duplicated host mentions, and on hand-written cases for T and the skip counts.  No device."""
import numpy as np
import pytest

from tests import cooccur_ref as R


def _random_mentions(rng, n_chunks, n, nnz):
    m = np.stack([rng.integers(0, n_chunks, nnz), rng.integers(0, n, nnz)], axis=1)
    return m, rng.integers(1, 9, nnz)


@pytest.mark.parametrize("weight", ["count", "product"])
def test_the_reference_equals_the_upper_triangle_of_the_gram_matrix(weight):
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(1)
    n_chunks, n = 300, 90
    m, w = _random_mentions(rng, n_chunks, n, 1500)
    row_ptr, ent, ww = R.csr_of(n_chunks, n, m, w)
    chunk = np.repeat(np.arange(n_chunks), np.diff(row_ptr))
    data = np.ones(len(ent), np.int64) if weight == "count" else ww.astype(np.int64)
    a = sp.csr_matrix((data, (chunk, ent.astype(np.int64))), shape=(n_chunks, n))
    gram = sp.triu(a.T @ a, k=1).tocoo()
    order = np.lexsort((gram.col, gram.row))
    got = R.cooccur(row_ptr, ent, ww, n, weight=weight, max_mentions=4096)
    assert np.array_equal(got.pairs, np.stack([gram.row[order], gram.col[order]], axis=1))
    assert np.array_equal(got.weights, gram.data[order]) and got.largest_weight == gram.data.max()
    d = np.diff(row_ptr)
    assert got.total_pairs == int((d * (d - 1) // 2).sum()) and got.chunks_skipped == 0 and got.entries_skipped == 0


def test_permuted_and_duplicated_host_mentions_give_the_same_answer():
    rng = np.random.default_rng(2)
    m, w = _random_mentions(rng, 50, 30, 400)
    want = R.cooccur_mentions(50, 30, m, w, weight="product")
    perm = rng.permutation(len(m))
    got = R.cooccur_mentions(50, 30, m[perm], w[perm], weight="product")
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # a mention given twice with half the weight each is the same mention
    even = w * 2
    twice = R.cooccur_mentions(50, 30, np.concatenate([m, m]), np.concatenate([w, w]), weight="product")
    once = R.cooccur_mentions(50, 30, m, even, weight="product")
    assert all(np.array_equal(a, b) for a, b in zip(twice, once))
    count = R.cooccur_mentions(50, 30, np.concatenate([m, m]), weight="count")
    assert all(np.array_equal(a, b) for a, b in zip(count, R.cooccur_mentions(50, 30, m, weight="count")))


def test_hand_written_cases():
    # chunk 0: {0, 1, 2}; chunk 1: {1, 2}; chunk 2: {5}; chunk 3: empty; chunk 4: {0, 1, 2, 3, 4}
    m = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 5), (4, 0), (4, 1), (4, 2), (4, 3), (4, 4)]
    w = [2, 3, 4, 5, 6, 7, 1, 1, 1, 1, 1]
    got = R.cooccur_mentions(5, 6, m, w)
    assert got.total_pairs == 3 + 1 + 10 and got.contributing == 3 and got.chunks_skipped == 0 and got.entries_skipped == 0
    assert got.pairs.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]]
    assert got.weights.tolist() == [2, 2, 1, 1, 3, 1, 1, 1, 1, 1] and got.largest_weight == 3
    got = R.cooccur_mentions(5, 6, m, w, weight="product", min_weight=8)
    assert got.pairs.tolist() == [[0, 2], [1, 2]] and got.weights.tolist() == [8 + 1, 12 + 30 + 1] and got.below_min_weight == 8
    got = R.cooccur_mentions(5, 6, m, w, max_mentions=4)                                 # the hub guard: chunk 4 gives nothing
    assert got.total_pairs == 4 and got.chunks_skipped == 1 and got.pairs.tolist() == [[0, 1], [0, 2], [1, 2]] and got.weights.tolist() == [1, 1, 2]
    got = R.cooccur_mentions(5, 6, m, w, max_mentions=2)
    assert got.total_pairs == 1 and got.chunks_skipped == 2 and got.contributing == 1 and got.pairs.tolist() == [[1, 2]]
    got = R.cooccur_mentions(5, 6, m, w, min_weight=4)                                   # above the largest W: an empty answer
    assert got.pairs.shape == (0, 2) and got.weights.shape == (0,) and got.largest_weight == 3 and got.below_min_weight == 10


def test_the_guards_of_a_raw_csr():
    # row 0: an entity >= n, a zero weight, a weight of 2^12, one good entry and an entity < 0; row 1: a repeated entity; row 2 reaches past nnz
    row_ptr = [0, 5, 8, 99]
    ent = [7, 1, 2, 3, -1, 4, 4, 5, 0, 6]
    w = [1, 0, 4096, 2, 1, 3, 3, 2, 1, 4095]
    got = R.cooccur(row_ptr, ent, w, 7, weight="product")
    assert got.entries_skipped == 4 and got.contributing == 2 and got.total_pairs == 3 + 1      # row 0 has one valid entry
    assert got.pairs.tolist() == [[0, 6], [4, 5]] and got.weights.tolist() == [4095, 12]         # (4, 4) gives nothing
    assert R.cooccur([0, 0, 0], [1], [1], 5).total_pairs == 0 and R.cooccur([0, 1], [1], [1], 5).pairs.shape == (0, 2)
