"""tests/components_ref.py, the restatement of the hook-and-jump rule, held against what does not share its code:
a plain union-find, scipy.sparse.csgraph.connected_components and networkx.connected_components.  The labels are the smallest
member of each component, and the rounds stay within ceil(log2 n) + 2 — on the scrambled path of 4097 vertices too, where plain
label propagation needs thousands."""
import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components as scipy_components

from tests import components_ref as R
from tests import ppr_ref


def _cases():
    cases = {"n2": (2, np.array([[0, 1]])), "two_and_isolated": ppr_ref.two_components_and_isolated(),
             "path_4097_scrambled": (4097, R.scrambled_path(4097, 7)), "path_in_order": (300, np.array(ppr_ref.path_graph(300))),
             "star": ppr_ref.star_graph(500), "star_clique_isolated": R.star_clique_isolated(300, 12, 9),
             "caterpillar": R.caterpillar_of_stars(16, 9), "edgeless": (7, np.zeros((0, 2), np.int64))}
    for seed, (n, m) in enumerate([(50, 20), (500, 300), (500, 2000), (3000, 2200)]):
        cases[f"random_{n}_{m}"] = (n, R.random_sparse(n, m, seed))
    return cases


CASES = _cases()


def _smallest_member(n, comp):
    """any component numbering -> the smallest vertex of each vertex's component"""
    first = np.full(int(comp.max()) + 1 if n else 0, n, np.int64)
    np.minimum.at(first, comp, np.arange(n))
    return first[comp]


@pytest.mark.parametrize("name", list(CASES))
def test_the_rule_equals_union_find_scipy_and_networkx(name):
    n, edges = CASES[name]
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    got = R.components(n, edges)
    assert np.array_equal(got["labels"], R.union_find(n, edges))
    a = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n))
    n_c, comp = scipy_components(a, directed=False)
    assert got["n_components"] == n_c and np.array_equal(got["labels"], _smallest_member(n, comp))
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges.tolist())
    want = np.empty(n, np.int64)
    for members in nx.connected_components(g):
        want[list(members)] = min(members)
    assert np.array_equal(got["labels"], want)
    # the summary: dense ids ascend with the labels, the sizes add up, the largest is the first of the largest
    assert np.array_equal(np.unique(got["labels"])[got["dense"]], got["labels"])
    assert got["sizes"].sum() == n and np.array_equal(got["sizes"], np.bincount(got["dense"], minlength=n_c))
    label, size = got["largest"]
    assert size == got["sizes"].max() and label == np.unique(got["labels"])[int(np.argmax(got["sizes"]))]


@pytest.mark.parametrize("name", list(CASES))
def test_the_rounds_stay_within_the_bound_and_every_round_starts_from_a_star_forest(name):
    n, edges = CASES[name]
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if not len(edges):
        assert R.components(n, edges)["rounds"] == 0
        return
    states = R.rounds_of(n, edges)
    assert 1 <= len(states) <= R.round_bound(n), (len(states), R.round_bound(n))
    for p in states:
        assert np.array_equal(p[p], p) and np.all(p <= np.arange(n))
    assert np.array_equal(states[-1], states[-2]) if len(states) > 1 else np.array_equal(states[0], np.arange(n))
    # the trees that still have an outside edge never grow in number and at least halve over two rounds (a local minimum nobody
    # hooked into — a leaf of a star whose hub is larger — sees only smaller roots in the next round and hooks then)
    left = [len(np.unique(p[edges][p[edges[:, 0]] != p[edges[:, 1]]])) for p in [np.arange(n)] + states]
    assert all(b <= a for a, b in zip(left, left[1:])) and all(c <= a // 2 for a, c in zip(left, left[2:])), left
    assert left[-1] == 0


def test_the_bound_and_what_it_is_there_to_fail():
    assert [R.round_bound(n) for n in (2, 3, 4, 5, 4096, 4097)] == [3, 4, 4, 5, 14, 15]
    n, edges = CASES["path_4097_scrambled"]
    assert R.components(n, edges)["rounds"] <= 15
    assert R.label_propagation_rounds(n, edges, 1000) == 1000            # plain label propagation is still going after 1000 rounds
    assert R.label_propagation_rounds(*CASES["star"], 10) == 2


def test_the_order_of_the_edges_and_the_direction_of_a_pair_do_not_matter():
    n, edges = CASES["random_3000_2200"]
    want = R.rounds_of(n, edges)
    rng = np.random.default_rng(1)
    shuffled = edges[rng.permutation(len(edges))]
    shuffled[::2] = shuffled[::2, ::-1]
    got = R.rounds_of(n, shuffled)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_the_generators():
    n, edges = R.star_clique_isolated()
    deg = np.bincount(edges.ravel(), minlength=n)
    assert n == 8321 and deg[0] == 8200 and sorted(set(deg.tolist())) == [0, 1, 69, 8200] and (deg == 0).sum() == 50
    n, edges = R.caterpillar_of_stars()
    assert n == 64 * 65 and len(edges) == 64 * 64 + 63
    first = R.rounds_of(n, edges)[0]
    hubs = np.arange(64) * 65 + 64
    assert R.components(n, edges)["n_components"] == 1 and np.all(first[hubs] == 0)       # the chain of 64 hooks, walked by one jump
    assert first[65] == 65 and len(R.rounds_of(n, edges)) == 3                            # the leaves follow in the second round
    x, chain, pairs = R.chain_embeddings()
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    sim = np.triu(xn @ xn.T, 1)
    assert np.array_equal(np.argwhere(sim >= 0.95), pairs)
    assert all(len(set(R.components(len(x), pairs)["labels"][chain == c])) == 1 for c in range(10))
    x, group = R.planted_duplicates()
    xn = x.astype(np.float64)
    sim = xn @ xn.T
    same = (group[:, None] == group[None, :]) & (group[:, None] >= 0)
    np.fill_diagonal(same, True)
    assert sim[same].min() > 0.99 and sim[~same].max() < 0.9
