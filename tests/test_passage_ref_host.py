"""tests/passage_ref.py — the fixed-point passage projection the kernels are held to, bit for bit — checked on its own: it does
not depend on the order of the mentions or on how a weight is split over duplicates, a batch is its rows, S stays below 2^40,
the floor costs less than 2^-28 against exact rational arithmetic, it agrees with float64 on networkx.pagerank inside a
derived bound, ties go to the smaller chunk and a chunk without mentions is never ranked."""
import random
from fractions import Fraction

import numpy as np

from tests import passage_ref as P
from tests import ppr_ref as R
from tests.test_ppr_ref_host import _l1_bound

N, N_CHUNKS = 200, 150
EDGES, WEIGHTS = R.random_graph(N, 600, seed=11, max_weight=5)
MENTIONS, MWEIGHTS = P.random_mentions(N, N_CHUNKS, seed=12)
SEEDS = [[3], [17, 150, 17], [5, 6, 7, 8], [199]]
STATES, _ = R.ppr(N, EDGES, SEEDS, weights=WEIGHTS)


def test_mention_order_and_split_weights_do_not_matter():
    want = [P.chunk_state(p, N_CHUNKS, MENTIONS, MWEIGHTS) for p in STATES]
    order = list(range(len(MENTIONS)))
    random.Random(1).shuffle(order)
    assert [P.chunk_state(p, N_CHUNKS, [MENTIONS[i] for i in order], [MWEIGHTS[i] for i in order]) for p in STATES] == want
    m2, w2 = P.split_weights(MENTIONS, MWEIGHTS, seed=2)
    assert len(m2) > len(MENTIONS) and P.merged(N_CHUNKS, N, m2, w2) == P.merged(N_CHUNKS, N, MENTIONS, MWEIGHTS)
    assert [P.chunk_state(p, N_CHUNKS, m2, w2) for p in STATES] == want


def test_a_batch_is_its_rows():
    batch, _ = R.ppr(N, EDGES, SEEDS, weights=WEIGHTS, tolerance=3e-3, max_iterations=30)
    for q, s in enumerate(SEEDS):
        p, _ = R.ppr_one(N, EDGES, s, weights=WEIGHTS, tolerance=3e-3, max_iterations=30)
        assert P.chunk_state(p, N_CHUNKS, MENTIONS, MWEIGHTS) == P.chunk_state(batch[q], N_CHUNKS, MENTIONS, MWEIGHTS)


def test_the_largest_state_stays_below_2_to_the_40():
    """one seed and damping 0 leave ALL the mass on the seed; a chunk mentioning it with the largest weight holds the largest S"""
    p, _ = R.ppr_one(N, EDGES, [9], weights=WEIGHTS, damping=0.0)
    assert p[9] == R.ONE and sum(p) == R.ONE
    S = P.chunk_state(p, 2, [(1, 9)], [P.MAX_WEIGHT - 1])
    assert S == [0, (P.MAX_WEIGHT - 1) << 28] and S[1] < 1 << 40
    assert ((S[1] << 24) | 0xFFFFFF) < 1 << 64                                  # the top-k key fits
    m2, w2 = [(1, 9)] * 3, [4000, 90, 5]                                         # the same weight split over duplicates
    assert P.chunk_state(p, 2, m2, w2) == S
    for q_state in STATES:                                                       # and nowhere near on ordinary states
        assert max(P.chunk_state(q_state, N_CHUNKS, MENTIONS, MWEIGHTS)) < 1 << 40


def test_the_floor_costs_less_than_one_unit_against_exact_rationals():
    for p in STATES:
        S = P.chunk_state(p, N_CHUNKS, MENTIONS, MWEIGHTS)
        exact = [Fraction(0)] * N_CHUNKS
        for (c, e), w in P.merged(N_CHUNKS, N, MENTIONS, MWEIGHTS).items():
            exact[c] += Fraction(w * p[e], R.ONE)
        for c, sc in enumerate(P.scores(S)):
            assert Fraction(sc) == Fraction(S[c], P.SCORE_ONE)                    # the float is exact
            assert 0 <= exact[c] - Fraction(sc) < Fraction(1, P.SCORE_ONE)


def test_against_float64_numpy_on_networkx():
    """|score(c) - sum_e w_ce want(e)| <= wmax(c) (L + n 1e-12) + 2^-28 + deg(c) wmax(c) 2^-52.

    With L the L1 bound of test_ppr_ref_host.py between p / ONE and the exact rule, and networkx within n tol = n 1e-12 of that
    rule in L1 (as that test allows): sum_e w_ce |p(e) / ONE - want(e)| <= wmax(c) sum_e |p(e) / ONE - want(e)| <= wmax(c)
    (L + n 1e-12) — each p is multiplied by at most the chunk's largest weight.  The >> 12 floors away less than one unit of
    2^-28.  The float64 dot product rounds deg(c) products and sums of magnitude <= wmax(c): deg(c) wmax(c) 2^-52 is generous."""
    import networkx as nx

    G = nx.connected_watts_strogatz_graph(120, 6, 0.2, seed=4)
    n, edges = 120, sorted((min(a, b), max(a, b)) for a, b in G.edges())
    _, W = R.adjacency(n, edges)
    damping = R.damping_q16(0.85) / 65536.0
    seeds, w = [4, 50, 77], [4, 1, 2]
    want = nx.pagerank(G, alpha=damping, personalization={4: 4.0, 50: 1.0, 77: 2.0}, tol=1e-12, max_iter=1000)
    p, _ = R.ppr_one(n, edges, seeds, w, damping=0.85, max_iterations=400)
    l1 = _l1_bound(n, W, damping, 400, len(seeds)) + n * 1e-12
    n_chunks = 60
    mentions, mw = P.random_mentions(n, n_chunks, seed=5)
    A = np.zeros((n_chunks, n), np.float64)
    for (c, e), x in P.merged(n_chunks, n, mentions, mw).items():
        A[c, e] = x
    ref = A @ np.asarray([want[v] for v in range(n)], np.float64)
    got = P.scores(P.chunk_state(p, n_chunks, mentions, mw))
    checked = 0
    for c in range(n_chunks):
        wmax, deg = A[c].max(), int((A[c] > 0).sum())
        assert abs(got[c] - ref[c]) <= wmax * l1 + 2.0 ** -28 + deg * wmax * 2.0 ** -52, c
        checked += deg > 0
    assert checked > 40


def test_ties_go_to_the_smaller_chunk_and_empty_chunks_are_never_ranked():
    mentions, weights = P.with_twins([(3, 7), (3, 9), (1, 7)], [5, 2, 1], src=3, dst=0)
    S = P.chunk_state(STATES[2], 5, mentions, weights)
    assert S[0] == S[3] > 0 and S[2] == S[4] == 0
    ids, sc, cnt = P.topk(S, 5)
    assert cnt == 3 and ids[3:] == [-1, -1] and sc[3:] == [float("-inf")] * 2
    assert ids.index(0) + 1 == ids.index(3)                                     # twins: adjacent, the smaller id first
    assert sc[:3] == sorted(sc[:3], reverse=True) and 2 not in ids and 4 not in ids
    assert P.topk(S, 1)[0] == ids[:1] and P.topk([0] * 5, 2) == ([-1, -1], [float("-inf")] * 2, 0)
    ms, ws = P.chunk_of_degree(N, 65, seed=3)
    assert len({e for _, e in ms}) == 65 and all(c == 0 for c, _ in ms)
