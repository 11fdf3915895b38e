"""tests/ppr_ref.py — the fixed-point personalized PageRank the kernels are held to, bit for bit — checked on its own: it does
not depend on the order of the edges, a batch is its rows, the floors cost no more than the derived bound against the same
rule in float64, mass is never created, and on a connected graph it agrees with networkx."""
import random

import pytest

from tests import ppr_ref as R

N300 = 300
EDGES300, WEIGHTS300 = R.random_graph(N300, 900, seed=7, max_weight=5)
SEEDS = [[3], [17, 200, 17], [5, 6, 7, 8], [299]]
SEED_W = [[1], [1 << 20, 1 << 19, 3], [10, 0, 1000, 7], [5]]


def _l1_bound(n, W, damping, iterations, slots):
    """|p_int / ONE - p_float|_1 <= ((sum_v W(v) + n) / (1 - damping) + 2 slots) 2^-40 + n T 2^-50.

    One integer step from the same p differs from the exact step as follows.  c(u) = p(u) // W(u) loses less than one unit,
    which v sees multiplied by w_uv: flow(v) loses less than sum_u w_uv = W(v) units.  The final >> 16 loses less than one
    unit more.  So one step floors fewer than W(v) + 1 units at v: sum_v (W(v) + 1) = sum W + n units of 2^-40 in L1.  The
    exact step is linear and contracts L1 by `damping` (the flow operator is column-stochastic), so the floors of T steps
    sum to less than (sum W + n) 2^-40 / (1 - damping).
    The teleport vector is floored too, once per seed slot: the integer t lies below the exact one by less than `slots` units
    in L1.  That is the distance of the two p_0 (it shrinks by `damping` per step: at most `slots` units ever), and every step
    adds (1 - damping) of it again, a geometric series that sums to less than `slots` units: 2 slots units in all — the
    constant the issue's formula leaves out.
    The float64 rule itself rounds: about n operations of relative 2^-53 on values <= 1 per step — n T 2^-50 is generous."""
    return ((sum(W) + n) / (1.0 - damping) + 2 * slots) * 2.0 ** -40 + n * iterations * 2.0 ** -50


def test_edge_order_and_pair_ends_do_not_matter():
    want, _ = R.ppr(N300, EDGES300, SEEDS, SEED_W, weights=WEIGHTS300)
    order = list(range(len(EDGES300)))
    random.Random(3).shuffle(order)
    edges = [EDGES300[i][::-1] if i % 2 else EDGES300[i] for i in order]
    got, _ = R.ppr(N300, edges, SEEDS, SEED_W, weights=[WEIGHTS300[i] for i in order])
    assert got == want


@pytest.mark.parametrize("tolerance", [0.0, 1e-4, 3e-3])
def test_a_batch_is_its_rows(tolerance):
    batch, its = R.ppr(N300, EDGES300, SEEDS, SEED_W, weights=WEIGHTS300, tolerance=tolerance, max_iterations=30)
    for q, (s, w) in enumerate(zip(SEEDS, SEED_W)):
        p, it = R.ppr_one(N300, EDGES300, s, w, weights=WEIGHTS300, tolerance=tolerance, max_iterations=30)
        assert p == batch[q] and it == its[q]
    if tolerance == 0.0:
        assert its == [30] * len(SEEDS)
    if tolerance == 3e-3:
        assert len(set(its)) > 1 and max(its) < 30          # the queries stop at different iterations


@pytest.mark.parametrize("damping", [0.0, 0.5, 0.85])
def test_the_floors_stay_inside_the_derived_l1_bound(damping):
    _, W = R.adjacency(N300, EDGES300, WEIGHTS300)
    for s, w in zip(SEEDS, SEED_W):
        p, _ = R.ppr_one(N300, EDGES300, s, w, weights=WEIGHTS300, damping=damping)
        f = R.ppr_float(N300, EDGES300, s, w, weights=WEIGHTS300, damping=damping)
        l1 = sum(abs(x / R.ONE - y) for x, y in zip(p, f))
        assert l1 <= _l1_bound(N300, W, R.damping_q16(damping) / 65536.0, 20, len(s))
        assert abs(sum(f) - 1.0) < 1e-12


def test_mass_is_never_created():
    adj, W = R.adjacency(N300, EDGES300, WEIGHTS300)
    for s, w in zip(SEEDS, SEED_W):
        t = R.teleport(N300, s, w)
        p = list(t)
        assert sum(p) <= R.ONE
        for _ in range(25):
            p = R.step(adj, W, t, p, R.damping_q16(0.85))
            assert 0 <= min(p) and sum(p) <= R.ONE
    n, edges = R.two_components_and_isolated()
    p, _ = R.ppr_one(n, edges, [0, 6, 10])
    assert sum(p) <= R.ONE


def test_an_isolated_seed_keeps_its_mass():
    n, edges = R.two_components_and_isolated()
    p, _ = R.ppr_one(n, edges, [11])
    assert p == [R.ONE if v == 11 else 0 for v in range(n)]
    p, _ = R.ppr_one(n, edges, [11, 0])
    assert p[11] == R.ONE // 2 and sum(p[6:]) == p[11] and 0 < sum(p[:6]) <= R.ONE // 2
    ids, sc, cnt = R.topk(p, 9)
    assert cnt == 7 and ids[0] == 11 and ids[7:] == [-1, -1] and sc[8] == float("-inf")


def test_zero_weights_and_unused_slots():
    n, edges = R.two_components_and_isolated()
    assert R.ppr_one(n, edges, [0, 3], [0, 0])[0] == [0] * n
    assert R.ppr_one(n, edges, [-1, -1])[0] == [0] * n
    assert R.topk([0] * n, 3) == ([-1] * 3, [float("-inf")] * 3, 0)
    assert R.ppr_one(n, edges, [2, -1, 2])[0] == R.ppr_one(n, edges, [2])[0] == R.ppr_one(n, edges, [2, 2], [7, 7])[0]
    assert R.quantise_weights([0.5, 0.25, 0.0]) == [1 << 20, 1 << 19, 0] and R.quantise_weights([0.0, 0.0]) == [0, 0]


def test_against_networkx_on_a_connected_graph():
    nx = pytest.importorskip("networkx")
    G = nx.connected_watts_strogatz_graph(120, 6, 0.2, seed=4)
    n, edges = 120, sorted((min(a, b), max(a, b)) for a, b in G.edges())
    _, W = R.adjacency(n, edges)
    damping = R.damping_q16(0.85) / 65536.0
    seeds, w = [4, 50, 77], [4, 1, 2]
    want = nx.pagerank(G, alpha=damping, personalization={4: 4.0, 50: 1.0, 77: 2.0}, tol=1e-12, max_iter=1000)
    p, _ = R.ppr_one(n, edges, seeds, w, damping=0.85, max_iterations=400)        # 0.85^400: far below the bound
    l1 = sum(abs(p[v] / R.ONE - want[v]) for v in range(n))
    assert l1 <= _l1_bound(n, W, damping, 400, len(seeds)) + n * 1e-12
