"""tests/ppr_ref.py's numpy sibling `ppr_batch` (and tests/passage_ref.py's `chunk_states_batch`) against the Python-integer
definitions they restate: equal element for element and in the iterations run.  The GPU tests of the larger shapes
(tests/test_gpu_ppr_forms.py) compare the kernels with the numpy forms; these tests are why they may."""
import random

import numpy as np
import pytest

from tests import passage_ref as P
from tests import ppr_ref as R

N300 = 300
EDGES300, WEIGHTS300 = R.random_graph(N300, 900, seed=7, max_weight=5)


def _seed_sets(n, count, rng):
    """`count` queries of 1 .. 6 seeds with integer weights; duplicates happen (as tests/test_gpu_ppr.py draws them)"""
    seeds = [[rng.randrange(n) for _ in range(rng.randint(1, 6))] for _ in range(count)]
    return seeds, [[rng.randint(1, 50) for _ in s] for s in seeds]


def _same(n, edges, seeds, seed_w=None, **kw):
    want, want_its = R.ppr(n, edges, seeds, seed_w, **kw)
    got, its = R.ppr_batch(n, edges, seeds, seed_w, **kw)
    assert got.dtype == np.uint64 and got.shape == (len(seeds), n)
    assert got.tolist() == want and list(its) == want_its
    return want, want_its


@pytest.mark.parametrize("damping", [0.0, 0.85])
def test_the_path(damping):
    _same(2, [(0, 1)], [[0], [1], [0, 1]], damping=damping)
    _same(5, R.path_graph(5), [[0], [2], [4, 0]], [[1 << 20], [5], [1 << 18, 1 << 20]], damping=damping)
    _same(40, R.path_graph(40), [[0], [39, 20], [7, 7, -1]], damping=damping, max_iterations=30)


@pytest.mark.parametrize("damping", [0.0, 0.85])
def test_isolated_seeds_and_a_query_without_weight(damping):
    n, edges = R.two_components_and_isolated()
    seeds = [[11], [11, 0], [0, 6, 10], [3, 4], [12, 12, 7], [-1, -1]]
    w = [[1], [1, 1], [2, 7, 1], [0, 0], [4, 2, 1], [1, 1]]
    want, _ = _same(n, edges, seeds, w, damping=damping)
    assert want[0][11] == R.ONE and want[3] == [0] * n and want[5] == [0] * n


@pytest.mark.parametrize("tolerance", [0.0, 3e-3])
@pytest.mark.parametrize("damping", [0.0, 0.85])
def test_the_random_weighted_graph(damping, tolerance):
    seeds, w = _seed_sets(N300, 24, random.Random(11))
    seeds += [[3], [299], [17, 200, 17]]
    w += [[1], [5], [1 << 20, 1 << 19, 3]]
    _, its = _same(N300, EDGES300, seeds, w, weights=WEIGHTS300, damping=damping, tolerance=tolerance, max_iterations=30)
    if tolerance and damping:
        assert len(set(its)) > 2 and max(its) < 30            # the queries freeze at different steps, each on its own
    elif damping:
        assert its == [30] * len(seeds)
    else:
        assert its == [1] * len(seeds)                          # damping 0: p' = t = p_0, so the first delta is 0 <= any tolerance


def test_no_step_at_all():
    seeds, w = _seed_sets(N300, 5, random.Random(2))
    want, its = _same(N300, EDGES300, seeds, w, weights=WEIGHTS300, max_iterations=0)
    assert its == [0] * 5 and want == [R.teleport(N300, s, x) for s, x in zip(seeds, w)]


def test_the_graph_with_a_hub_and_the_bipartite_builders():
    n, edges, weights = R.with_hub(N300, EDGES300, 70, WEIGHTS300, max_weight=5)
    assert n == 301 and len(edges) == 970 and R.degrees(n, edges)[300] == 70 and sorted(set(weights[900:])) == [1, 2, 3, 4, 5]
    assert edges[:900] == EDGES300 and edges[900] == (0, 300) and edges[-1] == (69, 300)
    _same(n, edges, [[300], [0], [5, 250]], weights=weights, max_iterations=6)
    n, edges = R.complete_bipartite(3, 70)
    deg = R.degrees(n, edges)
    assert n == 73 and len(edges) == 210 and deg[:3] == [70] * 3 and deg[3:] == [3] * 70
    _same(n, edges, [[0], [3], [1, 72]], max_iterations=4)


def test_the_numpy_projection_equals_the_python_one():
    n, n_chunks = 200, 150
    edges, weights = R.random_graph(n, 600, seed=11, max_weight=5)
    mentions, mweights = P.random_mentions(n, n_chunks, seed=12)
    m2, w2 = P.split_weights(mentions, mweights, seed=4)                              # repeated (chunk, entity): the weights add up
    big, bw = P.chunk_of_degree(n, 65, seed=21, chunk=7)
    seeds, w = _seed_sets(n, 9, random.Random(3))
    states, _ = R.ppr_batch(n, edges, seeds, w, weights=weights)
    for ms, ws in ((mentions, mweights), (m2, w2), (big, bw), ([(0, 1), (2, 3)], None)):
        got = P.chunk_states_batch(states, n_chunks, ms, ws)
        assert got.dtype == np.uint64 and got.tolist() == [P.chunk_state(p, n_chunks, ms, ws) for p in states.tolist()]
