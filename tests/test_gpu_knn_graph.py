"""knn_graph on the GPU (csrc/knn.hip through rag_arc_amd...graph_db.knn_graph) against the float64 oracle of tests/knn_ref.py.

Exact category: ids equal the oracle's in order and scores lie within 1e-12 — tests/test_knn_ref_host.py proves from the oracle
alone that the 1e-12 band excuses nothing on these inputs.  Tie category (duplicate clusters, one dimension, zero rows): the
band comparison knn_ref.compare plus the properties each case names."""
import os

import numpy as np
import pytest

from tests import knn_ref as R

pytestmark = pytest.mark.gpu

_FIRST, _LAST = (int(v) for v in os.environ.get("RARC_FUZZ_SEEDS", "0:10").split(":"))


def _knn(x, top_k, cutoff):
    from rag_arc_amd.encapsulation.database.graph_db import knn_graph

    return knn_graph(x, top_k=top_k, similarity_cutoff=cutoff, as_arrays=True)


def _exact(case):
    seed, n, d, top_k, cutoff, noise = case
    x = R.exact_input(case)
    want = R.knn_graph_f64(x, top_k, cutoff)
    R.assert_equal_in_order(_knn(x, top_k, cutoff), want, case)
    return want


@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: "n%d-d%d-k%d-c%g" % (c[1], c[2], c[3], c[4]))
def test_exact_cases(case):
    want = _exact(case)
    n, top_k = case[1], case[3]
    if n - 1 < top_k:
        assert want[2].max() <= n - 1 and np.all(want[0][:, n - 1:] == -1)          # fewer than K neighbours: padding


@pytest.mark.parametrize("seed", range(_FIRST, _LAST))
def test_exact_sweep(seed):
    _exact(R.fuzz_case(seed))


@pytest.fixture(scope="module")
def threshold_case():
    x, late, early = R.threshold_input()
    return x, R.cosine_matrix_f64(x), late, early


def test_nearest_neighbour_in_the_last_and_in_the_first_chunk(threshold_case):
    """n = 8193: a column sees the rows in chunks of 512, 2048 and the rest.  50 rows have their nearest neighbour among the last
    100 rows — it arrives when the threshold has risen twice — and 50 among the first 100.  Cutoff -1: only the rising threshold
    prunes."""
    x, sim, (late, tail), (early, head) = threshold_case
    got = _knn(x, 10, -1.0)
    R.assert_equal_in_order(got, R.knn_from_sim(sim, 10, -1.0), "threshold, cutoff -1")
    assert np.array_equal(got[0][late, 0], tail) and np.array_equal(got[0][early, 0], head)
    assert np.all(got[2] == 10)


def test_a_cutoff_almost_nothing_passes(threshold_case):
    x, sim, _, _ = threshold_case
    got = _knn(x, 10, 0.9999)
    want = R.knn_from_sim(sim, 10, 0.9999)
    assert R.band_rows(sim, 10, 0.9999) == 0
    R.assert_equal_in_order(got, want, "threshold, cutoff 0.9999")
    assert (got[2] == 0).mean() > 0.95


def test_duplicate_clusters_larger_than_k_and_than_the_first_lists():
    """600 scaled copies of 3 vectors: every row has ~200 neighbours at cosine 1 — more than top_k and more than the 64 entries the
    first lists hold, so the wrapper repeats with larger ones.  Which 10 of a cluster come back is decided in the last bits: the
    band comparison, and every score is 1 to 1e-12."""
    from unittest import mock

    from rag_arc_amd.hip import binding as B

    x = R.scaled_copies()
    lib = B.load_library()
    with mock.patch.object(lib, "rarc_knn_graph", wraps=lib.rarc_knn_graph) as spy:
        got = _knn(x, 10, 0.85)
    assert spy.call_count >= 2                                                       # the growth loop ran
    R.compare(got, R.cosine_matrix_f64(x), 10, 0.85, what="scaled copies")
    assert np.all(got[2] == 10) and np.max(np.abs(got[1] - 1.0)) <= 1e-12


def test_identical_copies_come_first_with_equal_bits():
    """40 bit-identical rows among 1000: for each copy the 39 others come first, their scores are the SAME BITS (one summation
    order wherever a pair is scored) and their ids therefore ascend."""
    x, at = R.identical_copies()
    got = _knn(x, 64, -1.0)
    R.compare(got, R.cosine_matrix_f64(x), 64, -1.0, what="identical copies")
    ids, cos, cnt = got
    for a in at:
        others = at[at != a]
        assert np.array_equal(ids[a, :39], others), a
        assert len(set(cos[a, :39].view(np.uint64).tolist())) == 1 and abs(cos[a, 0] - 1.0) <= 1e-12, a
        assert cnt[a] == 64
    assert len(set(cos[at, 0].view(np.uint64).tolist())) == 1                         # ... and the same bits in every copy's row


def test_one_dimension():
    x = R.one_dimension()
    for cutoff in (-1.0, 0.0, 0.85):
        got = _knn(x, 10, cutoff)
        R.compare(got, R.cosine_matrix_f64(x), 10, cutoff, what=("d = 1", cutoff))
        s = got[1][got[0] >= 0]                                                      # every cosine is -1, 0 or 1
        assert np.all(np.minimum(np.minimum(np.abs(s - 1.0), np.abs(s + 1.0)), np.abs(s)) <= 1e-12)


def test_zero_rows():
    x, z = R.with_zero_rows()
    sim = R.cosine_matrix_f64(x)
    ids, cos, cnt = _knn(x, 10, 0.85)
    R.compare((ids, cos, cnt), sim, 10, 0.85, what="zero rows, cutoff 0.85")
    assert np.all(cnt[z] == 0) and not np.isin(ids, z).any()                         # nobody's neighbour, no neighbours
    ids, cos, cnt = _knn(x, 10, 0.0)
    R.compare((ids, cos, cnt), sim, 10, 0.0, what="zero rows, cutoff 0")
    for r in z:                                                                       # everything ties at 0: the lowest ids
        assert np.array_equal(ids[r], [j for j in range(12) if j != r][:10]) and np.all(cos[r] == 0.0) and not np.signbit(cos[r]).any()


def test_surface():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import knn_graph
    from rag_arc_amd.hip.binding import RarcError, RarcUnsupported

    x = R.planted(3, 2000, 96, n_dup=200, noise=0.05)
    ids, cos, cnt = knn_graph(x, 10, 0.85, as_arrays=True)
    as_list = knn_graph(x, 10, 0.85)
    assert ids.dtype == np.int64 and cos.dtype == np.float64 and cnt.dtype == np.int32
    want = [(i, int(ids[i, t]), float(cos[i, t])) for i in range(len(x)) for t in range(cnt[i])]
    assert as_list == want and len(as_list) > 100
    assert all(type(i) is int and type(j) is int and type(s) is float for i, j, s in as_list)
    t = torch.from_numpy(x).cuda()
    before = t.clone()
    assert knn_graph(t, 10, 0.85) == as_list and torch.equal(t, before)               # a device tensor is used where it is
    wide = torch.zeros((2000, 128), dtype=torch.float32, device="cuda")
    wide[:, :96] = t
    assert knn_graph(wide[:, :96], 10, 0.85) == as_list                               # ... also a strided view (ld > d)
    d_ids, d_cos, d_cnt = knn_graph(x, as_arrays=True)                                # the defaults are GDS's: 10, 0.0
    assert d_ids.shape == (2000, 10) and np.all(d_cnt == 10) and d_cos.min() >= 0.0
    assert knn_graph([]) == [] and knn_graph([[1.0, 2.0]]) == []
    e = knn_graph([[1.0, 2.0]], 3, as_arrays=True)
    assert e[0].tolist() == [[-1, -1, -1]] and np.all(np.isneginf(e[1])) and e[2].tolist() == [0]
    assert knn_graph([[1.0, 0.0], [2.0, 0.0], [0.0, 0.0], [0.0, 1.0]], 2, 0.5) == [(0, 1, 1.0), (1, 0, 1.0)]
    with pytest.raises(ValueError):
        knn_graph(x, top_k=0)
    with pytest.raises(ValueError):
        knn_graph(x, similarity_cutoff=1.5)
    with pytest.raises(ValueError):
        knn_graph(x, similarity_cutoff=float("nan"))
    with pytest.raises(RarcUnsupported, match="256"):
        knn_graph(x, top_k=257)
    with pytest.raises(RarcError):
        knn_graph(np.zeros((3, 5000), dtype=np.float32))


def test_pairs_above_a_threshold_are_similar_pairs_bit_for_bit():
    """The undirected pairs of knn_graph(x, 256, 0.9) are similar_pairs(x, 0.9)'s (no row has more than 256 partners), and the
    scores are bit-equal: one exact arithmetic, one summation order."""
    from rag_arc_amd.encapsulation.database.graph_db import knn_graph, similar_pairs

    x = R.planted(9, 3000, 200, n_dup=600, noise=0.1)
    pairs = {(i, j): s for i, j, s in similar_pairs(x, 0.9)}
    ids, cos, cnt = knn_graph(x, 256, 0.9, as_arrays=True)
    assert cnt.max() < 256 and len(pairs) > 100
    edges = {}
    for i in range(len(x)):
        for t in range(cnt[i]):
            key = (min(i, int(ids[i, t])), max(i, int(ids[i, t])))
            assert edges.setdefault(key, float(cos[i, t])).hex() == float(cos[i, t]).hex(), key      # (i, j) and (j, i): same bits
    assert set(edges) == set(pairs)
    assert all(edges[k].hex() == float(pairs[k]).hex() for k in pairs)
