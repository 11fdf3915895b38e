"""Every batch form of the PageRank step (csrc/ppr.hip) on the GPU against tests/ppr_ref.py's `ppr_batch`, in full and bit for
bit.  tests/test_gpu_ppr.py reaches ppr_step_kernel<BP, QPL, SPLIT> at BP = 1, 4 and 64 with a hub of 65 neighbours; here are
the rest: every BP with and without the split form in one graph, two queries per lane in the split form, the third launch
(degree list 3: more than 8192 neighbours), every grid-stride walk (the plain and the split launch of the step, the init and
the transpose past their grid caps), and freezing under a tolerance in every form.  Each case asserts, from pagerank.limits(),
the degree classes and the graph's degrees, which form it reaches: a later change of a constant fails the case instead of
quietly moving it to another kernel.  DESIGN §4.13d lists instantiation x launch -> case.

The grid caps are not reported by the library; they are restated here from ppr.hip's launchers."""
import random

import numpy as np
import pytest

from tests import ppr_ref as R

pytestmark = pytest.mark.gpu

WAVE = 64                          # lanes of a wave: a lane is a query in the query-parallel form
PLAIN_CAP_WAVES = 8192 * 4         # ppr_launch_step: the launch over every vertex, 8192 workgroups of 4 waves, an item a wave
SPLIT_CAP_GROUPS = 2048            # ppr_launch_step: a launch over a degree list, an item a workgroup
INIT_CAP_THREADS = 4096 * 256      # rarc_ppr_seed: ppr_init_kernel, an element of the state a thread
TRANSPOSE_CAP_TILES = 8192         # rarc_ppr_scores / rarc_ppr_topk: a 64 x 64 tile a workgroup


def _limits():
    from rag_arc_amd.encapsulation.database.graph_db.communities import bucket_limits
    from rag_arc_amd.encapsulation.database.graph_db.pagerank import limits

    lim = limits()
    lim["list3_degree"] = bucket_limits()["lds"]               # a vertex of more neighbours is on degree list 3
    assert lim["split_degree"] == bucket_limits()["wave"]      # ... and of more than this on list 2: the split launches walk those lists
    return lim


def _form(batch, lim):
    """(BP, QPL, chunks of queries) of the instantiation rarc_ppr_step picks for a batch"""
    if batch > lim["vertex_parallel_max_batch"]:
        qpl = 2 if batch > WAVE and batch % 2 == 0 else 1
        return WAVE, qpl, -(-batch // (WAVE * qpl))
    bp = 1
    while bp < batch:
        bp *= 2
    return bp, 1, 1


def _graph(n, edges, weights=None):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, edges, weights=weights)


def _seed_sets(n, count, rng):
    """`count` queries of 1 .. 6 seeds with integer weights; duplicates happen"""
    seeds = [[rng.randrange(n) for _ in range(rng.randint(1, 6))] for _ in range(count)]
    return seeds, [[rng.randint(1, 50) for _ in s] for s in seeds]


def _check(g, n, edges, seeds, seed_w, weights=None, k=None, rows=(), **kw):
    """scores in full and bit for bit; with k, the ids, scores and counts of `rows` -> (the reference states, iterations run)"""
    sw = None if seed_w is None else [R.quantise_weights(w) for w in seed_w]
    want, its = R.ppr_batch(n, edges, seeds, sw, weights=weights, **kw)
    got = g.personalized_pagerank(seeds, seed_w, **kw)
    assert got.dtype == np.float64 and got.shape == (len(seeds), n)
    assert np.array_equal(got, want.astype(np.float64) / 2.0 ** 40)          # p <= 2^40: both steps exact
    if k is not None:
        ids, sc, cnt = g.personalized_pagerank(seeds, seed_w, top_k=k, **kw)
        assert ids.shape == (len(seeds), k) and sc.shape == (len(seeds), k) and cnt.shape == (len(seeds),)
        for q in rows:
            wi, wsc, wc = R.topk(want[q].tolist(), k)
            assert cnt[q] == wc and ids[q].tolist() == wi and sc[q].tolist() == wsc, (k, q)
    return want, its


# ---- every instantiation, plain and split in one graph ---------------------------------------------------------------------------------
HUB, HUB_DEGREE = 300, 70


@pytest.fixture(scope="module")
def hub300():
    """random_graph(300, 900) with weights 1 .. 5 and vertex 300 joined to the vertices 0 .. 69 with weights 1 .. 5"""
    edges, weights = R.random_graph(300, 900, seed=7, max_weight=5)
    n, edges, weights = R.with_hub(300, edges, HUB_DEGREE, weights, max_weight=5)
    return {"n": n, "edges": edges, "weights": weights, "deg": R.degrees(n, edges), "g": _graph(n, edges, weights)}


EVERY_BATCH = [2, 4, 5, 8, 9, 16, 17, 32, 33, 63, 66, 128, 129, 255, 256]


def test_the_batches_reach_every_instantiation_and_the_graph_both_launches(hub300):
    lim, deg = _limits(), hub300["deg"]
    forms = {_form(b, lim)[:2] for b in EVERY_BATCH}
    assert forms == {(2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2)}      # BP = 1 is B = 1: the list 3 case below
    assert {_form(b, lim)[2] for b in EVERY_BATCH} == {1, 2, 3, 4}                    # ... and every count of query chunks
    assert lim["split_degree"] < deg[HUB] == HUB_DEGREE <= lim["list3_degree"]        # the hub: the split launch over list 2
    rest = deg[:HUB]
    assert max(rest) <= lim["split_degree"] and min(rest) >= 1                        # everyone else: the plain launch ...
    assert any(d <= 8 for d in rest) and any(9 <= d <= lim["split_degree"] for d in rest)       # ... its tail loop alone, and the unrolled one
    assert lim["max_batch"] == 256


@pytest.mark.parametrize("batch", EVERY_BATCH)
def test_every_instantiation_plain_and_split(hub300, batch):
    """query 0 seeds the hub itself, query 1 one of its neighbours; the rest are random sets, which reach both as well"""
    n = hub300["n"]
    seeds, w = _seed_sets(n, batch, random.Random(1000 + batch))
    seeds[0], w[0] = [HUB], [1]
    seeds[1], w[1] = [5, 200], [3, 1]
    assert hub300["deg"][HUB] > _limits()["split_degree"] and (5, HUB) in hub300["edges"]
    k = 10 if batch in (2, 16, 66) else None
    want, _ = _check(hub300["g"], n, hub300["edges"], seeds, w, weights=hub300["weights"], k=k, rows=sorted({0, 1, batch // 2, batch - 1}))
    assert want[0][:HUB_DEGREE].all() and want[1][HUB] > 0          # the split launch wrote the hub's row and the plain one read it


# ---- degree list 3: the third launch -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k3_8193():
    n, edges = R.complete_bipartite(3, 8193)
    return {"n": n, "edges": edges, "g": _graph(n, edges)}


def _bipartite_seeds(n, batch, rng):
    """a left vertex, a right vertex, a mix of both; then random sets over all vertices"""
    seeds, w = _seed_sets(n, batch, rng)
    for q, (s, x) in enumerate((([0], [1]), ([n - 2], [1]), ([2, n - 5, 1, n - 1], [3, 1, 2, 7]))):
        if q < batch:
            seeds[q], w[q] = s, x
    return seeds, w


@pytest.mark.parametrize("batch", [1, 2, 3, 6, 9, 17, 65, 130])
def test_three_vertices_on_degree_list_3(k3_8193, batch):
    """K(3, 8193): the three left vertices have 8193 neighbours, one more than list 2 takes.  The launch over list 3 has
    (n / 8192 + 1) * chunks = 2 * chunks workgroups for 3 * chunks items: it is also the strided split walk, a wave keeping
    its chunk of queries.  B = 1, 2, 3, 6, 9, 17: BP = 1, 2, 4, 8, 16, 32; 65: a lane a query, two chunks; 130: two queries
    per lane — every instantiation once."""
    lim, n = _limits(), k3_8193["n"]
    assert 8193 > lim["list3_degree"] and n == 8196
    bp, qpl, chunks = _form(batch, lim)
    assert (bp, qpl, chunks) == {1: (1, 1, 1), 2: (2, 1, 1), 3: (4, 1, 1), 6: (8, 1, 1), 9: (16, 1, 1), 17: (32, 1, 1), 65: (64, 1, 2),
                                 130: (64, 2, 2)}[batch]
    assert (n // lim["list3_degree"] + 1) * chunks < 3 * chunks            # fewer workgroups than items: the third left vertex is a second visit
    seeds, w = _bipartite_seeds(n, batch, random.Random(2000 + batch))
    want, _ = _check(k3_8193["g"], n, k3_8193["edges"], seeds, w, k=5 if batch == 6 else None, rows=range(min(batch, 6)), max_iterations=3)
    assert want[0][:3].all() and want[0][3:].all()                          # the left vertices took mass from every right one and back


def test_degree_8192_stays_on_list_2():
    """K(3, 8192), one below: the left vertices are the largest list 2 takes, and the launch over list 3 runs over an empty list"""
    lim = _limits()
    n, edges = R.complete_bipartite(3, 8192)
    assert 8192 == lim["list3_degree"] and min(n - 1, len(edges)) > lim["list3_degree"]       # the launcher's degree bound: list 3 is launched
    seeds, w = _bipartite_seeds(n, 6, random.Random(2100))
    _check(_graph(n, edges), n, edges, seeds, w, k=5, rows=range(6), max_iterations=3)


# ---- the strided walks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [65, 130])
def test_a_strided_split_launch_over_list_2(batch):
    """K(65, 1100): every vertex is split (1100 of degree 65, 65 of degree 1100): 1165 * 2 chunks = 2330 items for 2048 workgroups"""
    lim = _limits()
    n, edges = R.complete_bipartite(65, 1100)
    deg = R.degrees(n, edges)
    chunks = _form(batch, lim)[2]
    assert chunks == 2 and _form(batch, lim)[1] == (2 if batch == 130 else 1)
    assert lim["split_degree"] < min(deg) and max(deg) <= lim["list3_degree"]
    assert n * chunks > SPLIT_CAP_GROUPS and SPLIT_CAP_GROUPS % chunks == 0
    seeds, w = _bipartite_seeds(n, batch, random.Random(3000 + batch))
    want, _ = _check(_graph(n, edges), n, edges, seeds, w, max_iterations=3)
    assert want[0].all()                                       # the list's order is the device's: whichever vertex came late carries mass


@pytest.mark.parametrize("n,batch", [(17000, 65), (17000, 129), (33000, 3)])
def test_a_strided_plain_launch_and_a_strided_init(n, batch):
    """a path of n vertices, seeds at both ends and in the middle.  (17000, 65): 2 chunks, 34000 items for 32768 waves, and
    1.1 M elements for the init's 1 M threads; (17000, 129): 3 chunks, the grid rounded up past its cap to a multiple of 3;
    (33000, 3): the vertex-parallel form, one chunk"""
    lim = _limits()
    chunks = _form(batch, lim)[2]
    assert chunks == {65: 2, 129: 3, 3: 1}[batch] and n * chunks > PLAIN_CAP_WAVES
    assert (n * batch > INIT_CAP_THREADS) == (batch != 3)
    first_late = PLAIN_CAP_WAVES // chunks                      # the first vertex some wave reaches on its second visit (at most)
    assert first_late + 8 < n
    edges = R.path_graph(n)
    rng = random.Random(4000 + batch)
    seeds, w = _seed_sets(n, batch, rng)
    seeds[0], seeds[1], seeds[2] = [0], [n - 1], [n // 2, n - 2, 0]
    w[0], w[1], w[2] = [1], [1], [5, 2, 1]
    for q in range(3, batch, 3):
        seeds[q][0] = rng.randrange(first_late + 8, n)
    want, _ = _check(_graph(n, edges), n, edges, seeds, w, max_iterations=3)
    late = want[:, first_late + 8:]
    assert late[1].any() and late[2].any() and not late[0].any() and late.any(axis=1).sum() >= batch // 3


def test_a_strided_transpose():
    """a path of 530000 vertices at B = 1: 8282 tiles of 64 vertices for 8192 workgroups, for the scores and for the top-k keys"""
    n = 530000
    tiles = -(-n // 64)
    assert tiles == 8282 > TRANSPOSE_CAP_TILES and n < 1 << 24
    edges = R.path_graph(n)
    seeds, w = [[0, n // 2, n - 1, n - 3]], [[1, 2, 3, 1]]
    want, _ = _check(_graph(n, edges), n, edges, seeds, w, k=5, rows=(0,), max_iterations=2)
    assert want[0][TRANSPOSE_CAP_TILES * 64:].any() and max(R.topk(want[0].tolist(), 5)[0]) >= TRANSPOSE_CAP_TILES * 64


# ---- freezing in every form ----------------------------------------------------------------------------------------------------------
def _freezing_seeds(f, batch):
    """even queries: one seed on a vertex of at most three neighbours (slow to settle); odd ones: six random seeds (quick);
    query 2 seeds the hub.  Fixed: the counts asserted below are the reference's own"""
    low = [v for v in range(f["n"]) if 1 <= f["deg"][v] <= 3]
    rng = random.Random(50 + batch)
    seeds = [[low[(q // 2) % len(low)]] if q % 2 == 0 else [rng.randrange(f["n"]) for _ in range(6)] for q in range(batch)]
    seeds[2] = [HUB]
    return seeds


@pytest.mark.parametrize("batch", [6, 24, 40, 130])
def test_queries_freeze_on_their_own_in_every_form(hub300, batch):
    """B = 6 and 24: vertex-parallel, the lanes of one neighbour slot differ in `live`; 40: a lane a query; 130: two queries
    per lane, one frozen while the other runs.  The hub's row goes through the split form in each"""
    lim, n, g = _limits(), hub300["n"], hub300["g"]
    assert _form(batch, lim)[:2] == {6: (8, 1), 24: (32, 1), 40: (64, 1), 130: (64, 2)}[batch]
    seeds = _freezing_seeds(hub300, batch)
    kw = {"tolerance": 3e-3, "max_iterations": 30}
    want, its = _check(g, n, hub300["edges"], seeds, None, weights=hub300["weights"], **kw)
    assert len(set(its)) > 2 and max(its) < 30
    if batch == 130:
        assert sum(its[2 * j] != its[2 * j + 1] for j in range(batch // 2)) > batch // 4       # lanes with one half frozen
    else:
        assert its[0] != its[1]                                # (every query of a batch up to 64 is in one wave)
    got = g.personalized_pagerank(seeds, **kw)
    for q in sorted({0, 1, 2, its.index(min(its)), its.index(max(its)), batch - 1}):
        assert np.array_equal(g.personalized_pagerank([seeds[q]], **kw)[0], got[q])
