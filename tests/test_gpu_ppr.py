"""EntityGraph.personalized_pagerank / retrieve on the GPU (csrc/ppr.hip) against the integer restatement tests/ppr_ref.py:
the fixed-point state p (read back through rarc_ppr_scores as p / 2^40, exact) and the top-k ids, scores and counts are equal
bit for bit — the rule is integer arithmetic, so there is no band.  The shapes are small ones that reach both forms of the
step — of ppr_step_kernel<BP, QPL, SPLIT>, BP = 1, 4 and 64 (B = 1, 3 and 40 .. 130) on the random graph, BP = 2 and 8 only
in passing (two device-side queries, five on 13 vertices, seven in retrieve) — a partial wave and a second one, the 16-byte
form, a hub one below, at and above the degree at which a vertex is split across a workgroup (B = 1, 3, 64, 65: one query
per lane), isolated vertices, duplicated and unused seed slots, a query without weight.  Every instantiation on one graph
(BP = 16 and 32 run nowhere here), the split form at every BP and with two queries per lane, the launch over degree list 3,
the grid-stride walks and freezing outside B = 40 live in tests/test_gpu_ppr_forms.py."""
import random

import numpy as np
import pytest

from tests import ppr_ref as R

pytestmark = pytest.mark.gpu


def _graph(n, edges, weights=None):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, edges, weights=weights)


def _seed_sets(n, count, rng):
    """`count` queries of 1 .. 6 seeds with integer weights; duplicates happen"""
    seeds = [[rng.randrange(n) for _ in range(rng.randint(1, 6))] for _ in range(count)]
    return seeds, [[rng.randint(1, 50) for _ in s] for s in seeds]


def _ref_weights(ws):
    """what the Python layer makes of float weights: scaled to the largest, round(w * 2^20)"""
    return [R.quantise_weights(w) for w in ws]


def _check(n, edges, seeds, seed_w, weights=None, ks=(), **kw):
    """scores bit for bit, then every k of ks: ids, scores, counts"""
    want, _ = R.ppr(n, edges, seeds, None if seed_w is None else _ref_weights(seed_w), weights=weights, **kw)
    g = _graph(n, edges, weights)
    got = g.personalized_pagerank(seeds, seed_w, **kw)
    assert got.dtype == np.float64 and got.shape == (len(seeds), n)
    assert np.array_equal(got, np.asarray([R.scores(p) for p in want]))
    for k in ks:
        ids, sc, cnt = g.personalized_pagerank(seeds, seed_w, top_k=k, **kw)
        assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int32
        for q, p in enumerate(want):
            wi, wsc, wc = R.topk(p, k)
            assert cnt[q] == wc and ids[q].tolist() == wi and sc[q].tolist() == wsc, (k, q)
    return want


def test_one_edge_and_a_path():
    for damping in (0.0, 0.85):
        _check(2, [(0, 1)], [[0], [1], [0, 1]], None, ks=(1, 2, 3), damping=damping)
        _check(5, R.path_graph(5), [[0], [2], [4, 0]], [[1.0], [0.3], [0.25, 1.0]], ks=(1, 5, 8), damping=damping)


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("batch", [1, 3, 64, 65])
def test_a_hub_around_the_split_degree(delta, batch):
    """a star whose hub has one neighbour fewer than a single wave walks, exactly as many, and one more (the split form)"""
    from rag_arc_amd.encapsulation.database.graph_db.pagerank import limits

    leaves = limits()["split_degree"] + delta
    n, edges = R.star_graph(leaves)
    rng = random.Random(100 + delta)
    seeds, w = _seed_sets(n, batch, rng)
    seeds[0], w[0] = [0], [1]                                 # the hub itself
    _check(n, edges, seeds, w, ks=(4,), max_iterations=5)


def test_components_isolated_vertices_and_a_query_without_weight():
    n, edges = R.two_components_and_isolated()
    seeds = [[11], [11, 0], [0, 6, 10], [3, 4], [12, 12, 7]]
    w = [[1.0], [1.0, 1.0], [0.2, 0.7, 0.1], [0.0, 0.0], [1.0, 0.5, 0.25]]
    want = _check(n, edges, seeds, w, ks=(1, n, n + 4))
    assert want[0][11] == R.ONE and want[3] == [0] * n          # all the mass on one vertex; none at all
    assert R.topk(want[3], 3)[2] == 0 and R.topk(want[1], n)[2] == 7


@pytest.fixture(scope="module")
def g300():
    edges, weights = R.random_graph(300, 900, seed=7, max_weight=5)
    return 300, edges, weights


@pytest.mark.parametrize("batch", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("damping", [0.0, 0.85])
def test_a_random_weighted_graph_in_every_form(g300, batch, damping):
    """B = 1 and 3: vertex-parallel; 64: query-parallel, one full wave; 65: a second, partial wave; 130: two queries per lane"""
    n, edges, weights = g300
    seeds, w = _seed_sets(n, batch, random.Random(batch))
    _check(n, edges, seeds, w, weights=weights, ks=(1, 10, n, n + 7) if batch <= 3 else (10,), damping=damping)


def test_one_slot_and_sixty_four_slots_with_a_duplicate(g300):
    n, edges, weights = g300
    rng = random.Random(9)
    many = [rng.randrange(n) for _ in range(63)]
    many.append(many[5])
    _check(n, edges, [[7], many, [8]], [[2.0], [rng.random() for _ in many], [0.1]], weights=weights, ks=(20,))


def test_permuted_edges_give_the_same_bits(g300):
    n, edges, weights = g300
    seeds, w = _seed_sets(n, 40, random.Random(1))
    want = _graph(n, edges, weights).personalized_pagerank(seeds, w)
    order = list(range(len(edges)))
    random.Random(2).shuffle(order)
    got = _graph(n, [edges[i][::-1] if i % 3 == 0 else edges[i] for i in order], [weights[i] for i in order]).personalized_pagerank(seeds, w)
    assert np.array_equal(got, want)


def test_queries_freeze_on_their_own_under_a_tolerance(g300):
    n, edges, weights = g300
    seeds = [[3], [17, 200, 17], [5, 6, 7, 8], [299]] + _seed_sets(n, 36, random.Random(4))[0]
    want, its = R.ppr(n, edges, seeds, weights=weights, tolerance=3e-3, max_iterations=30)
    assert len(set(its)) > 2 and max(its) < 30
    g = _graph(n, edges, weights)
    got = g.personalized_pagerank(seeds, tolerance=3e-3, max_iterations=30)
    assert np.array_equal(got, np.asarray([R.scores(p) for p in want]))
    for q in (0, 1, 39):
        assert np.array_equal(g.personalized_pagerank([seeds[q]], tolerance=3e-3, max_iterations=30)[0], got[q])


def test_a_batch_of_300_is_its_rows(g300):
    n, edges, weights = g300
    seeds, w = _seed_sets(n, 300, random.Random(5))
    g = _graph(n, edges, weights)
    got = g.personalized_pagerank(seeds, w, max_iterations=6)
    ids, sc, cnt = g.personalized_pagerank(seeds, w, max_iterations=6, top_k=5)
    assert got.shape == (300, n) and ids.shape == (300, 5)
    for q in list(range(0, 300, 23)) + [255, 256, 299]:
        one = g.personalized_pagerank([seeds[q]], [w[q]], max_iterations=6)
        assert np.array_equal(one[0], got[q])
        oi, osc, oc = g.personalized_pagerank([seeds[q]], [w[q]], max_iterations=6, top_k=5)
        assert oi[0].tolist() == ids[q].tolist() and osc[0].tolist() == sc[q].tolist() and oc[0] == cnt[q]
    want, _ = R.ppr(n, edges, seeds[250:260], _ref_weights(w[250:260]), weights=weights, max_iterations=6)
    assert np.array_equal(got[250:260], np.asarray([R.scores(p) for p in want]))


def test_device_inputs_and_outputs(g300):
    import torch

    n, edges, weights = g300
    g = _graph(n, torch.from_numpy(np.asarray(edges, dtype=np.int64)).cuda(), weights)
    seeds = torch.tensor([[4, 9, -1], [250, -1, -1]], dtype=torch.int64).cuda()
    out = g.personalized_pagerank(seeds, as_device=True)
    assert out.is_cuda and out.dtype == torch.float64
    want, _ = R.ppr(n, edges, [[4, 9, -1], [250, -1, -1]], weights=weights)
    assert np.array_equal(out.cpu().numpy(), np.asarray([R.scores(p) for p in want]))
    ids, sc, cnt = g.personalized_pagerank(seeds, top_k=3, as_device=True)
    assert ids.is_cuda and sc.is_cuda and cnt.is_cuda and ids[0].tolist() == R.topk(want[0], 3)[0]


def test_retrieve_seeds_from_the_index_then_ranks(g300):
    """row i of a 200 x 64 fp16 index is vertex i: the seeds are index.search's own answer and the ranking is ppr_ref's"""
    from rag_arc_amd.hip.engine import FlatIndexF16

    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 64)).astype(np.float32)
    x[:, 0] += 6.0                                            # every row leans towards e0: a query along -e0 scores them all below 0
    e0 = np.zeros((1, 64), np.float32)
    e0[0, 0] = 1.0
    queries = np.concatenate([x[:3] + 0.1 * rng.standard_normal((3, 64)).astype(np.float32), -e0, e0,
                              rng.standard_normal((2, 64)).astype(np.float32)])
    index = FlatIndexF16(64, metric="cosine", device=0)
    index.add(x)
    edges, _ = R.random_graph(200, 500, seed=8)
    g = _graph(200, edges)
    D, I = index.search(queries, 5)
    ids, sc, cnt = g.retrieve(index, queries, seeds_per_query=5, top_k=10)
    for q in range(len(queries)):
        w = R.quantise_weights(np.clip(D[q].astype(np.float64), 0.0, None))
        p, _ = R.ppr_one(200, edges, I[q].tolist(), w)
        wi, wsc, wc = R.topk(p, 10)
        assert ids[q].tolist() == wi and sc[q].tolist() == wsc and cnt[q] == wc
    assert I[:3, 0].tolist() == [0, 1, 2] and (D[:3, 0] > 0.9).all()      # a near-duplicate leads its query's seeds
    assert (D[3] < 0).all() and cnt[3] == 0 and ids[3].tolist() == [-1] * 10      # scores clipped at 0: a query without weight
    other = FlatIndexF16(64, metric="cosine", device=0)
    other.add(x[:150])
    with pytest.raises(ValueError, match="150 rows"):
        g.retrieve(other, queries)


def test_refusals_come_before_any_launch(g300):
    from unittest import mock

    from rag_arc_amd.encapsulation.database.graph_db import pagerank
    from rag_arc_amd.hip import binding as B

    n, edges, weights = g300
    g = _graph(n, edges, weights)
    refusing = mock.Mock(side_effect=AssertionError("a launch"))
    with mock.patch.object(g, "_run", refusing):
        for seeds, kw in (([list(range(65))], {}), ([], {}), ([[n]], {}), ([[-2]], {}), ([[0.5]], {}), ([[1]], {"seed_weights": [[-1.0]]}),
                          ([[1]], {"seed_weights": [[float("nan")]]}), ([[1]], {"seed_weights": [[float("inf")]]}),
                          ([[1]], {"damping": 1.0}), ([[1]], {"damping": -0.1}), ([[1]], {"top_k": 0}), ([[1]], {"top_k": 8193}),
                          ([[1]], {"tolerance": -1.0}), ([[1]], {"max_iterations": -1})):
            with pytest.raises(ValueError):
                g.personalized_pagerank(seeds, **kw)
        import torch

        with pytest.raises(ValueError):
            g.personalized_pagerank(torch.zeros((2, 65), dtype=torch.int64).cuda())
        with pytest.raises(ValueError):
            g.personalized_pagerank(torch.full((1, 2), n, dtype=torch.int64).cuda())
        with mock.patch.object(g, "n", 1 << 24):              # the argument check suffices: nothing that large is allocated
            with pytest.raises(B.RarcUnsupported, match="2\\^24"):
                g.personalized_pagerank([[1]], top_k=5)
    assert not refusing.called
    assert B.load_library().rarc_ppr_workspace_bytes(n, len(edges), 0) == 0
    assert pagerank.MAX_SEEDS == 64
