"""louvain_communities / entity_clusters on the GPU (csrc/louvain.hip) against the integer restatement tests/louvain_ref.py:
the labels are equal element for element — the rule is integer arithmetic and a maximum of (G, -label), so there is no band.
The inputs are the smallest that reach each form of the kernels: every degree class of the sweep, several levels (the aggregate
and loop weights), the mover bit, ties on every gain, and the global-memory table."""
import random

import numpy as np
import pytest

from tests import louvain_ref as R

pytestmark = pytest.mark.gpu


def _gpu(n, edges, **kw):
    from rag_arc_amd.encapsulation.database.graph_db import louvain_communities

    return louvain_communities(n, edges, **kw).tolist()


def _barabasi_albert():
    nx = pytest.importorskip("networkx")
    G = nx.barabasi_albert_graph(3000, 3, seed=3)
    return 3000, R.normalise(3000, G.edges())


def _planted():
    nx = pytest.importorskip("networkx")
    G = nx.planted_partition_graph(20, 50, .3, .005, seed=1)
    return 1000, R.normalise(1000, G.edges())


CASES = {
    "path3": lambda: (3, R.path_graph(3)),
    "edge": lambda: (2, [(0, 1)]),
    "matching": lambda: (64, [(2 * i, 2 * i + 1) for i in range(32)]),
    "cliques": lambda: R.disjoint_cliques([2, 3, 5, 8, 40, 1, 1]),
    "k30-30": lambda: R.complete_bipartite(30, 30),
    "ring": lambda: R.ring_of_cliques(30, 5),
    "path200": lambda: (200, R.path_graph(200)),
    "cycle64": lambda: (64, R.cycle_graph(64)),
    "grid40": lambda: R.grid_graph(40, 40),
    "barabasi-albert": _barabasi_albert,
    "planted-20x50": _planted,
    "clique600": lambda: (600, R.clique(0, 600)),
    "star-and-triangles": lambda: R.star_and_triangles(20000, 200),
}
_REF = {}


def _case(name):
    """(n, edges, the reference's labels, its trace): computed once per session, never modified"""
    if name not in _REF:
        n, edges = CASES[name]()
        trace = []
        _REF[name] = (n, edges, R.louvain(n, edges, trace=trace), trace)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_labels_equal_the_reference(name):
    n, edges, want, trace = _case(name)
    assert _gpu(n, edges) == want
    if name == "ring":
        assert R.levels_run(trace) >= 2                      # the aggregate and loop weights are exercised
    if name in ("path200", "cycle64", "grid40", "barabasi-albert"):
        assert R.levels_run(trace) >= 4
    if name == "cliques":
        assert sorted(len(c) for c in R.clusters_from_labels(want, 1)) == [1, 1, 2, 3, 5, 8, 40]
    if name == "k30-30":
        assert want == list(range(n))


def test_degree_classes_of_the_cases():
    """Which form each case reaches follows from the bucket constants: the 600-clique sits in the LDS-table class with a tie on
    every gain, the star's hub meets 20,000 distinct communities in sweep 0 — more than the LDS table's class holds — and takes
    the global-memory table, its leaves and the triangles the 8-lane form, the planted partition the wave form."""
    from rag_arc_amd.encapsulation.database.graph_db.communities import bucket_limits

    lim = bucket_limits()
    assert lim["wave"] < 599 <= lim["lds"]
    assert 20000 > lim["lds"] and 2 * 20000 > lim["lds_slots"]
    n, edges, _, _ = _case("planted-20x50")
    deg = np.bincount(np.asarray(edges).ravel(), minlength=n)
    assert ((deg > lim["group"]) & (deg <= lim["wave"])).sum() > n // 2
    n, edges, _, _ = _case("barabasi-albert")
    deg = np.bincount(np.asarray(edges).ravel(), minlength=n)
    assert (deg <= lim["group"]).any() and ((deg > lim["group"]) & (deg <= lim["wave"])).any() and (deg > lim["wave"]).any()


@pytest.mark.parametrize("name", ["ring", "grid40", "star-and-triangles"])
def test_shuffled_edges_and_pairs_on_the_device(name):
    import torch

    n, edges, want, _ = _case(name)
    shuffled = [(b, a) if i % 3 == 0 else (a, b) for i, (a, b) in enumerate(edges)]
    random.Random(11).shuffle(shuffled)
    assert _gpu(n, shuffled + shuffled[:7]) == want           # swapped ends and duplicates are normalised on the host
    dev = torch.from_numpy(np.asarray(sorted(edges, key=lambda e: (e[1] * 7919 + e[0]) % 1009), dtype=np.int64)).cuda()
    assert _gpu(n, dev) == want
    with pytest.raises(ValueError):
        _gpu(n, torch.flip(dev, dims=[1]))                    # device pairs are used where they are: i < j is required


@pytest.mark.parametrize("name", ["path200", "ring", "barabasi-albert"])
@pytest.mark.parametrize("kw", [{"max_iterations": 1}, {"max_levels": 1}, {"max_iterations": 3, "max_levels": 2}], ids=str)
def test_limits_on_sweeps_and_levels(name, kw):
    n, edges, full, _ = _case(name)
    want = R.louvain(n, edges, **kw)
    assert _gpu(n, edges, **kw) == want
    if "max_levels" in kw:
        assert want != full


def test_nothing_to_cluster_launches_nothing():
    from unittest import mock

    from rag_arc_amd.encapsulation.database.graph_db import communities

    with mock.patch.object(communities.B, "load_library", side_effect=AssertionError("a launch")):
        assert communities.louvain_communities(5, []).tolist() == [0, 1, 2, 3, 4]
        assert communities.louvain_communities(1, []).tolist() == [0]
        assert communities.louvain_communities(0, np.zeros((0, 2), np.int64)).tolist() == []


# ---- entity_clusters ---------------------------------------------------------------------------------------------------------------
GROUP_SIZES = [1, 1, 2, 3, 5, 17, 64, 300, 1]


@pytest.fixture(scope="module")
def planted_groups():
    """d = 64; each group a random unit vector plus 0.01 N(0, I) per row, rows permuted.  Within a group the cosine is >= 0.988,
    across groups <= 0.334 (asserted below from the float64 matrix): the 0.95 graph is disjoint cliques."""
    rng = np.random.default_rng(5)
    rows, group = [], []
    for g, size in enumerate(GROUP_SIZES):
        c = rng.standard_normal(64)
        c /= np.linalg.norm(c)
        rows.append(c + 0.01 * rng.standard_normal((size, 64)))
        group += [g] * size
    x = np.concatenate(rows)
    perm = rng.permutation(len(x))
    return x[perm].astype(np.float32), np.asarray(group)[perm]


def test_entity_clusters_are_the_planted_groups(planted_groups):
    from rag_arc_amd.encapsulation.database.graph_db import entity_clusters

    x, group = planted_groups
    xn = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    sim = xn @ xn.T
    same = group[:, None] == group[None, :]
    assert sim[same].min() >= 0.988 and sim[~same].max() <= 0.334
    members = [np.nonzero(group == g)[0].tolist() for g in range(len(GROUP_SIZES))]
    want_all = sorted(members, key=lambda m: (-len(m), m[0]))
    want = [m for m in want_all if len(m) >= 2]
    assert [len(m) for m in want] == [300, 64, 17, 5, 3, 2]
    assert entity_clusters(x) == want
    assert entity_clusters(x.tolist(), min_size=1) == want_all
    assert entity_clusters(x, min_size=6) == want[:3]
    labels = entity_clusters(x, as_labels=True)
    assert labels.dtype == np.int64 and labels.shape == (len(x),)
    assert R.clusters_from_labels(labels, 2) == want
    assert all(labels[m].tolist() == [m[0]] * len(m) for m in members)


def test_entity_clusters_on_chains_equal_the_reference_on_the_oracle_s_pairs(oracle):
    """Chains A ~ B ~ C with A !~ C at the threshold: consecutive rows 15 degrees apart (cosine 0.966), rows two steps apart 30
    degrees (0.866), each chain in a plane of its own — the case in which communities and connected components may differ.  The
    expected labels are the reference's on the float64 oracle's pairs."""
    from rag_arc_amd.encapsulation.database.graph_db import entity_clusters

    lengths = [3, 4, 5, 6, 3, 6, 4, 5, 6, 6]
    rows = []
    for c, length in enumerate(lengths):
        for s in range(length):
            v = np.zeros(2 * len(lengths))
            v[2 * c], v[2 * c + 1] = np.cos(np.radians(15.0 * s)), np.sin(np.radians(15.0 * s))
            rows.append((1.0 + 0.25 * s) * v)                 # any scale: the rows are normalised
    x = np.asarray(rows)[np.random.default_rng(2).permutation(len(rows))].astype(np.float32)
    pairs = [(i, j) for i, j, _ in oracle.similar_pairs_f64(x.astype(np.float64), 0.95)]
    assert len(pairs) == sum(length - 1 for length in lengths)
    want = R.louvain(len(x), R.normalise(len(x), pairs))
    got = entity_clusters(x, as_labels=True)
    assert got.tolist() == want
    assert entity_clusters(x) == R.clusters_from_labels(want, 2)
    assert len(set(want)) >= len(lengths)
