"""Typed personalized PageRank on the GPU (csrc/ppr.hip's TYPED step and seed over rarc_graph_types_weighted's slot arrays,
DESIGN §4.13m) against tests/typed_ppr_ref.py, in full and bit for bit: every instantiation <BP, QPL> of the step with and
without the split form, the third launch, two queries of different filters in one lane and in neighbouring lanes, filter 0 and
all ones, a neighbour nobody may reach, freezing, the strided walk, batches cut at 256, the chunk projection, seeds from an
index, and the blob the typed k-hop calls share.  Each case asserts, from pagerank.limits(), the degree classes and the graph's
degrees, which form it reaches (DESIGN §4.13m lists case -> launch)."""
import random

import numpy as np
import pytest

from tests import khop_ref as K
from tests import passage_ref as C
from tests import ppr_ref as R
from tests import typed_ppr_ref as TP
from tests import typed_ref as T

pytestmark = pytest.mark.gpu

WAVE = 64
PLAIN_CAP_WAVES = 8192 * 4         # ppr_launch_step: the launch over every vertex, 8192 workgroups of 4 waves, an item a wave
N_TYPES = 4
ALL = TP.ALL


def _limits():
    from rag_arc_amd.encapsulation.database.graph_db.communities import bucket_limits
    from rag_arc_amd.encapsulation.database.graph_db.pagerank import limits

    lim = limits()
    lim["list3_degree"] = bucket_limits()["lds"]               # a vertex of more neighbours is on degree list 3
    assert lim["split_degree"] == bucket_limits()["wave"]      # ... and of more than this on list 2: the split launches walk those lists
    return lim


def _form(batch, lim):
    """(BP, QPL, chunks of queries) of the instantiation rarc_ppr_step_typed picks for a batch: rarc_ppr_step's"""
    if batch > lim["vertex_parallel_max_batch"]:
        qpl = 2 if batch > WAVE and batch % 2 == 0 else 1
        return WAVE, qpl, -(-batch // (WAVE * qpl))
    bp = 1
    while bp < batch:
        bp *= 2
    return bp, 1, 1


def _popcount(x):
    return bin(int(x)).count("1")


def _rows(edges, masks, weights):
    """the input of EntityGraph(types=): a pair of mask M and weight w as one row per type of M, the weight spread over them
    (w >= popcount(M)), rows shuffled and every other one swapped — the constructor ORs the types and adds the weights back"""
    rows, types, ws = [], [], []
    for (a, b), mk, w in zip(edges, masks, weights):
        bits = [t for t in range(32) if int(mk) >> t & 1]
        assert 1 <= len(bits) <= w
        for i, t in enumerate(bits):
            rows.append((a, b))
            types.append(t)
            ws.append(w - (len(bits) - 1) if i == 0 else 1)
    order = list(range(len(rows)))
    random.Random(len(rows)).shuffle(order)
    return [rows[i][::-1] if i % 2 else rows[i] for i in order], [types[i] for i in order], [ws[i] for i in order]


def _graph(n, edges, masks, weights):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    if weights is None:
        rows, types, _ = _rows(edges, masks, [32] * len(edges))
        return EntityGraph(n, rows, types=types)
    rows, types, ws = _rows(edges, masks, weights)
    return EntityGraph(n, rows, weights=ws, types=types)


def _seed_sets(n, count, rng):
    """`count` queries of 1 .. 6 seeds with integer weights; duplicates happen"""
    seeds = [[rng.randrange(n) for _ in range(rng.randint(1, 6))] for _ in range(count)]
    return seeds, [[rng.randint(1, 50) for _ in s] for s in seeds]


def _filters(count, rng, n_types=N_TYPES):
    return [rng.randrange(1, 1 << n_types) for _ in range(count)]


def _check(f, seeds, seed_w, filters, k=None, rows=(), **kw):
    """scores in full and bit for bit; with k, the ids, scores and counts of `rows` -> (the reference states, iterations run)"""
    g, n = f["g"], f["n"]
    sw = None if seed_w is None else [R.quantise_weights(w) for w in seed_w]
    want, its = TP.ppr_batch(n, f["edges"], f["masks"], seeds, filters, sw, weights=f["weights"], **kw)
    rt = np.array(filters, np.uint32)
    got = g.personalized_pagerank(seeds, seed_w, relation_types=rt, **kw)
    assert got.dtype == np.float64 and got.shape == (len(seeds), n)
    assert np.array_equal(got, want.astype(np.float64) / 2.0 ** 40)          # p <= 2^40: both steps exact
    if k is not None:
        ids, sc, cnt = g.personalized_pagerank(seeds, seed_w, top_k=k, relation_types=rt, **kw)
        assert ids.shape == (len(seeds), k) and sc.shape == (len(seeds), k) and cnt.shape == (len(seeds),)
        for q in rows:
            wi, wsc, wc = R.topk(want[q].tolist(), k)
            assert cnt[q] == wc and ids[q].tolist() == wi and sc[q].tolist() == wsc, (k, q)
    return want, its


# ---- every instantiation, plain and split in one graph ---------------------------------------------------------------------------------
HUB, HUB_DEGREE = 300, 70


@pytest.fixture(scope="module")
def hub300():
    """300 random vertices, 900 pairs of random multi-bit masks over four types and weights up to 7, and vertex 300 joined to
    the vertices 0 .. 69 by edges whose single types alternate 0, 1, 2, 3"""
    edges, masks, weights = TP.random_typed_weighted(300, 900, N_TYPES, seed=7)
    weights = [max(w, _popcount(mk)) for w, mk in zip(weights, masks)]
    n, edges, masks, weights = TP.with_typed_hub(300, edges, masks, weights, HUB_DEGREE, N_TYPES)
    assert max(weights) == 7 and masks.min() > 0 and any(_popcount(mk) > 1 for mk in masks)
    return {"n": n, "edges": edges, "masks": masks, "weights": weights, "deg": R.degrees(n, edges), "g": _graph(n, edges, masks, weights)}


EVERY_BATCH = [1, 2, 3, 6, 9, 24, 40, 63, 66, 129, 130]


def test_the_batches_reach_every_instantiation_and_the_graph_both_launches(hub300):
    lim, deg = _limits(), hub300["deg"]
    forms = {_form(b, lim)[:2] for b in EVERY_BATCH}
    assert forms == {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2)}
    assert {_form(b, lim)[2] for b in EVERY_BATCH} == {1, 2, 3}
    assert lim["split_degree"] < deg[HUB] == HUB_DEGREE <= lim["list3_degree"]        # the hub: the split launch over list 2
    rest = deg[:HUB]
    assert max(rest) <= lim["split_degree"] and min(rest) >= 1                        # everyone else: the plain launch ...
    assert any(d <= 8 for d in rest) and any(9 <= d <= lim["split_degree"] for d in rest)       # ... its tail loop alone, and the unrolled one
    # the hub's allowed degree differs per query: 18 edges of types 0 and 1, 17 of types 2 and 3
    hub = {f: TP.allowed_degrees(hub300["n"], hub300["edges"], hub300["masks"], f)[HUB] for f in (1, 2, 4, 8, 3, 15)}
    assert hub == {1: 18, 2: 18, 4: 17, 8: 17, 3: 36, 15: 70}


@pytest.mark.parametrize("batch", EVERY_BATCH)
def test_every_instantiation_plain_and_split(hub300, batch):
    """query 0 seeds the hub itself under one type, query 1 one of its neighbours; the rest are random sets and filters"""
    n = hub300["n"]
    rng = random.Random(1000 + batch)
    seeds, w = _seed_sets(n, batch, rng)
    filters = _filters(batch, rng)
    seeds[0], w[0], filters[0] = [HUB], [1], 0b0010
    if batch > 1:
        seeds[1], w[1], filters[1] = [5, 200], [3, 1], 0b0011
    assert hub300["deg"][HUB] > _limits()["split_degree"] and (5, HUB) in hub300["edges"]
    k = 10 if batch in (2, 24, 66) else None
    want, _ = _check(hub300, seeds, w, filters, k=k, rows=sorted({0, min(1, batch - 1), batch // 2, batch - 1}))
    reached = [v for v in range(HUB_DEGREE) if want[0][v]]
    assert set(range(1, HUB_DEGREE, 4)) <= set(reached)           # the split launch wrote the hub's row under type 1 ...
    if batch > 1:
        assert want[1][HUB] > 0                                   # ... and the plain one read it: 5 - HUB has type 1
        assert len(set(filters)) > 1


@pytest.mark.parametrize("damping", [0.0, 0.5])
def test_other_dampings(hub300, damping):
    rng = random.Random(77)
    seeds, w = _seed_sets(hub300["n"], 9, rng)
    want, _ = _check(hub300, seeds, w, _filters(9, rng), k=5, rows=range(9), damping=damping)
    if damping == 0.0:
        assert [int(x.sum()) > 0 for x in want] == [True] * 9 and all((x > 0).sum() <= 6 for x in want)      # p = t


# ---- degree list 3: the third launch -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k3_8193():
    """K(3, 8193), the edge (i, 3 + j) of type (i + j) % 2, unit weights"""
    n, edges = R.complete_bipartite(3, 8193)
    masks = np.array([1 << ((a + b - 3) % 2) for a, b in edges], np.uint32)
    return {"n": n, "edges": edges, "masks": masks, "weights": None, "g": _graph(n, edges, masks, None)}


@pytest.mark.parametrize("batch", [1, 6, 65, 130])
def test_three_vertices_on_degree_list_3(k3_8193, batch):
    lim, n = _limits(), k3_8193["n"]
    assert 8193 > lim["list3_degree"] and n == 8196
    assert _form(batch, lim) == {1: (1, 1, 1), 6: (8, 1, 1), 65: (64, 1, 2), 130: (64, 2, 2)}[batch]
    rng = random.Random(2000 + batch)
    seeds, w = _seed_sets(n, batch, rng)
    filters = [(1, 2, 3)[q % 3] for q in range(batch)]
    for q, (s, x) in enumerate((([0], [1]), ([n - 2], [1]), ([2, n - 5, 1, n - 1], [3, 1, 2, 7]))):
        if q < batch:
            seeds[q], w[q] = s, x
    want, _ = _check(k3_8193, seeds, w, filters, k=5 if batch == 6 else None, rows=range(min(batch, 6)), max_iterations=3)
    # query 0 (filter {0}) from left vertex 0 reaches the even right vertices only, and through them left vertex 2 but not 1
    assert want[0][3::2].all() and not want[0][4::2].any() and want[0][0] and want[0][2] and not want[0][1]


# ---- two filters in one lane, and in neighbouring lanes ------------------------------------------------------------------------------
def _shut_in(f):
    """(vertex, type): a vertex none of whose edges carries the type — seeded under that type alone it keeps its mass"""
    allowed = [TP.allowed_degrees(f["n"], f["edges"], f["masks"], 1 << t) for t in range(N_TYPES)]
    for v in range(f["n"] - 1):
        for t in range(N_TYPES):
            if allowed[t][v] == 0 and f["deg"][v] >= 2:
                return v, t
    raise AssertionError("no vertex without a type")


@pytest.mark.parametrize("batch", [130, 6])
def test_neighbouring_queries_hold_different_filters(hub300, batch):
    """B = 130: queries 2 i and 2 i + 1 share a lane (QPL = 2); B = 6: neighbouring lanes of one neighbour slot (BP = 8).  Every
    even query runs under the one type its seed has no edge of, every odd one from the same seed under another filter"""
    lim = _limits()
    assert _form(batch, lim)[:2] == {130: (64, 2), 6: (8, 1)}[batch]
    v, t = _shut_in(hub300)
    rng = random.Random(batch)
    others = [f for f in range(1, 16) if f != 1 << t]
    seeds = [[v] if q % 4 < 2 else [v, rng.randrange(hub300["n"])] for q in range(batch)]
    filters = [1 << t if q % 2 == 0 else others[(q // 2) % len(others)] for q in range(batch)]
    want, _ = _check(hub300, seeds, None, filters, k=3, rows=(0, 1, batch - 2, batch - 1))
    for q in range(0, batch, 4):
        assert want[q][v] == R.ONE and (want[q] > 0).sum() == 1           # nothing leaves v
    lone = [q for q in range(1, batch, 4) if TP.allowed_degrees(hub300["n"], hub300["edges"], hub300["masks"], filters[q])[v]]
    assert lone and all((want[q] > 0).sum() > 10 and want[q][v] < R.ONE for q in lone)        # ... while its lane-mate spreads out


# ---- filter 0, all ones, and a neighbour nobody may reach ----------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [9, 66])
def test_filter_zero_and_all_ones_beside_ordinary_ones(hub300, batch):
    n, g = hub300["n"], hub300["g"]
    rng = random.Random(300 + batch)
    seeds, w = _seed_sets(n, batch, rng)
    filters = _filters(batch, rng)
    for q in range(0, batch, 3):
        filters[q] = ALL
    for q in range(1, batch, 3):
        filters[q] = 0
    want, _ = _check(hub300, seeds, w, filters, k=4, rows=(0, 1, 2, batch - 1))
    untyped = g.personalized_pagerank(seeds, w)
    typed = g.personalized_pagerank(seeds, w, relation_types=np.array(filters, np.uint32))
    for q in range(0, batch, 3):
        assert np.array_equal(typed[q], untyped[q])                         # every mask is non-zero: all ones is the untyped call
    for q in range(1, batch, 3):
        assert want[q].tolist() == R.teleport(n, seeds[q], R.quantise_weights(w[q]))      # filter 0: p = t
    assert any(not np.array_equal(typed[q], untyped[q]) for q in range(2, batch, 3))


@pytest.mark.parametrize("batch", [1, 9, 66, 130])
def test_a_neighbour_no_filter_of_the_batch_allows(hub300, batch):
    """every query under type 3 alone: the slots whose mask lacks it — most of the hub's — are met by no filter of any lane, so
    their rows of c are not loaded.  One iterable of ids is one filter for every query"""
    n = hub300["n"]
    lacking = sum(1 for mk in hub300["masks"] if not int(mk) & 8)
    assert lacking > len(hub300["masks"]) // 3
    seeds, w = _seed_sets(n, batch, random.Random(400 + batch))
    seeds[0], w[0] = [HUB], [1]
    sw = [R.quantise_weights(x) for x in w]
    want, _ = TP.ppr_batch(n, hub300["edges"], hub300["masks"], seeds, [8] * batch, sw, weights=hub300["weights"])
    got = hub300["g"].personalized_pagerank(seeds, w, relation_types=[3])
    assert np.array_equal(got, want.astype(np.float64) / 2.0 ** 40)
    assert want[0][3:HUB_DEGREE:4].all() and (want[0] > 0).sum() < (hub300["g"].personalized_pagerank([seeds[0]], [w[0]])[0] > 0).sum()


# ---- freezing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [6, 40, 130])
def test_queries_freeze_on_their_own(hub300, batch):
    """even queries: one seed on a vertex of at most three neighbours (slow to settle); odd ones: six random seeds (quick); the
    filters go round {0}, {1}, all, {2, 3}, none.  Rows must equal the one-query calls"""
    lim, n, g = _limits(), hub300["n"], hub300["g"]
    assert _form(batch, lim)[:2] == {6: (8, 1), 40: (64, 1), 130: (64, 2)}[batch]
    low = [v for v in range(n) if 1 <= hub300["deg"][v] <= 3]
    rng = random.Random(50 + batch)
    seeds = [[low[(q // 2) % len(low)]] if q % 2 == 0 else [rng.randrange(n) for _ in range(6)] for q in range(batch)]
    seeds[2] = [HUB]
    filters = [(1, 2, ALL, 12, 0)[q % 5] for q in range(batch)]
    kw = {"tolerance": 3e-3, "max_iterations": 30}
    want, its = _check(hub300, seeds, None, filters, **kw)
    assert len(set(its)) > 2 and min(its) == its[4] == 1 and sorted(its)[len(its) // 2] < 30      # (a filtered component may never settle)
    if batch == 130:
        assert sum(its[2 * j] != its[2 * j + 1] for j in range(batch // 2)) > batch // 4       # lanes with one half frozen
    got = g.personalized_pagerank(seeds, relation_types=np.array(filters, np.uint32), **kw)
    for q in sorted({0, 1, 2, 4, its.index(min(its)), its.index(max(its)), batch - 1}):
        alone = g.personalized_pagerank([seeds[q]], relation_types=np.array([filters[q]], np.uint32), **kw)
        assert np.array_equal(alone[0], got[q])


# ---- the strided walk, and batches cut at 256 ----------------------------------------------------------------------------------------
def test_a_strided_plain_launch():
    """a path of 17000 vertices, types alternating along it, B = 65: 2 chunks, 34000 items for 32768 waves"""
    lim = _limits()
    n, batch = 17000, 65
    chunks = _form(batch, lim)[2]
    assert chunks == 2 and n * chunks > PLAIN_CAP_WAVES
    first_late = PLAIN_CAP_WAVES // chunks
    edges = R.path_graph(n)
    masks = np.array([1 << (a % 2) for a, _ in edges], np.uint32)
    f = {"n": n, "edges": edges, "masks": masks, "weights": None, "g": _graph(n, edges, masks, None)}
    rng = random.Random(4065)
    seeds, w = _seed_sets(n, batch, rng)
    filters = [(3, 1, 2)[q % 3] for q in range(batch)]
    seeds[0], seeds[1], seeds[2] = [n - 1], [n - 1], [n - 1]
    w[0], w[1], w[2] = [1], [1], [1]
    for q in range(3, batch, 3):
        seeds[q][0] = rng.randrange(first_late + 8, n)
    want, _ = _check(f, seeds, w, filters, max_iterations=3)
    late = want[:, first_late + 8:]
    assert late.any(axis=1).sum() >= batch // 3
    # the last edge has type (n - 2) % 2 = 0, the one before type 1: from the end vertex three steps reach four vertices under
    # both types, its one neighbour and no further under {0}, nothing under {1}
    assert (want[1] > 0).sum() == 2 and (want[2] > 0).sum() == 1 and (want[0] > 0).sum() == 4


def test_300_queries_of_mixed_filters_are_cut_with_their_filters(hub300):
    n = hub300["n"]
    rng = random.Random(9)
    seeds, w = _seed_sets(n, 300, rng)
    filters = [rng.randrange(0, 16) for _ in range(300)]
    filters[255], filters[256], filters[299] = 1, 2, 4
    _check(hub300, seeds, w, filters, k=7, rows=(0, 255, 256, 299))


def test_permuted_pairs_give_the_same_bits(hub300):
    f = hub300
    order = list(range(len(f["edges"])))
    random.Random(5).shuffle(order)
    g2 = _graph(f["n"], [f["edges"][i][::-1] for i in order], f["masks"][order], [f["weights"][i] for i in order])
    rng = random.Random(6)
    seeds, w = _seed_sets(f["n"], 24, rng)
    filters = np.array(_filters(24, rng), np.uint32)
    a = f["g"].personalized_pagerank(seeds, w, relation_types=filters)
    b = g2.personalized_pagerank(seeds, w, relation_types=filters)
    assert np.array_equal(a, b) and a.any()


# ---- seeds, weights and how the graph was built --------------------------------------------------------------------------------------
def test_64_seed_slots_with_a_duplicate(hub300):
    n = hub300["n"]
    rng = random.Random(64)
    full = rng.sample(range(n), 63)
    full.append(full[10])
    seeds = [full, [HUB] * 64, [7]]
    w = [[rng.randint(1, 50) for _ in range(64)], [1] * 64, [1]]
    want, _ = _check(hub300, seeds, w, [0b0101, 0b1000, 0b0001], k=8, rows=range(3))
    assert (want[0] > 0).sum() > 64


def test_unit_weights_and_a_graph_adopted_from_device_buffers(hub300):
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    f = hub300
    rng = random.Random(11)
    seeds, w = _seed_sets(f["n"], 17, rng)
    filters = _filters(17, rng)
    # weights=None: the weight pointer of rarc_graph_types_weighted is null
    rows, types, _ = _rows(f["edges"], f["masks"], [32] * len(f["edges"]))
    unit = {**f, "weights": None, "g": EntityGraph(f["n"], rows, types=types)}
    assert unit["g"]._pair_weights is None
    _check(unit, seeds, w, filters, k=5, rows=(0, 16))
    # from_device: the masks handed over as they are, multi-bit included; with weights and without
    pairs = torch.from_numpy(np.array(f["edges"], np.int64)).cuda()
    md = torch.from_numpy(f["masks"].view(np.int32)).cuda()
    wd = torch.from_numpy(np.array(f["weights"], np.uint32).view(np.int32)).cuda()
    _check({**f, "g": EntityGraph.from_device(f["n"], pairs, wd, type_masks=md)}, seeds, w, filters, k=5, rows=(0, 16))
    _check({**unit, "g": EntityGraph.from_device(f["n"], pairs, type_masks=md)}, seeds, w, filters)


def test_the_one_shot_form(hub300):
    from rag_arc_amd.encapsulation.database.graph_db.pagerank import personalized_pagerank

    f = hub300
    rows, types, ws = _rows(f["edges"], f["masks"], f["weights"])
    seeds = [[3], [HUB, 9]]
    want, _ = TP.ppr_batch(f["n"], f["edges"], f["masks"], seeds, [2, 12], weights=f["weights"])
    got = personalized_pagerank(f["n"], rows, seeds, weights=ws, types=types, relation_types=[[1], [2, 3]])
    assert np.array_equal(got, want.astype(np.float64) / 2.0 ** 40)


# ---- chunks, and seeds from an index -------------------------------------------------------------------------------------------------
def test_rank_chunks_under_filters(hub300):
    from rag_arc_amd.encapsulation.database.graph_db.passages import MentionMap

    f, nc = hub300, 60
    mentions, mw = C.random_mentions(f["n"], nc, seed=5, max_weight=200)
    mm = MentionMap(nc, f["n"], mentions, weights=mw)
    for batch in (5, 66):
        rng = random.Random(500 + batch)
        seeds, w = _seed_sets(f["n"], batch, rng)
        filters = _filters(batch, rng)
        filters[1] = 0
        sw = [R.quantise_weights(x) for x in w]
        states, _ = TP.ppr_batch(f["n"], f["edges"], f["masks"], seeds, filters, sw, weights=f["weights"])
        S = TP.chunk_states(states, nc, mentions, mw)
        rt = np.array(filters, np.uint32)
        got = f["g"].rank_chunks(mm, seeds, w, relation_types=rt)
        assert np.array_equal(got, S.astype(np.float64) / 2.0 ** 28)
        ids, sc, cnt = f["g"].rank_chunks(mm, seeds, w, top_k=6, relation_types=rt)
        for q in (0, 1, batch - 1):
            wi, wsc, wc = C.topk(S[q].tolist(), 6)
            assert ids[q].tolist() == wi and sc[q].tolist() == wsc and cnt[q] == wc
        assert not np.array_equal(got, f["g"].rank_chunks(mm, seeds, w))


def test_retrieve_and_retrieve_chunks_seed_from_the_index_under_filters(hub300):
    from rag_arc_amd.encapsulation.database.graph_db.passages import MentionMap
    from rag_arc_amd.hip.engine import FlatIndexF16

    f, nc = hub300, 60
    n = f["n"]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, 64)).astype(np.float32)
    queries = np.concatenate([x[:3] + 0.1 * rng.standard_normal((3, 64)).astype(np.float32), rng.standard_normal((4, 64)).astype(np.float32)])
    index = FlatIndexF16(64, metric="cosine", device=0)
    index.add(x)
    D, I = index.search(queries, 5)
    mentions, mw = C.random_mentions(n, nc, seed=6, max_weight=200)
    mm = MentionMap(nc, n, mentions, weights=mw)
    filters = [1, 2, 4, 8, 3, 0, ALL]
    sw = [R.quantise_weights(np.clip(D[q].astype(np.float64), 0.0, None)) for q in range(7)]
    states, _ = TP.ppr_batch(n, f["edges"], f["masks"], [I[q].tolist() for q in range(7)], filters, sw, weights=f["weights"])
    S = TP.chunk_states(states, nc, mentions, mw)
    rt = np.array(filters, np.uint32)
    ids, sc, cnt = f["g"].retrieve(index, queries, seeds_per_query=5, top_k=10, relation_types=rt)
    cids, csc, ccnt = f["g"].retrieve_chunks(index, queries, mm, seeds_per_query=5, top_k=10, relation_types=rt)
    for q in range(7):
        wi, wsc, wc = R.topk(states[q].tolist(), 10)
        assert ids[q].tolist() == wi and sc[q].tolist() == wsc and cnt[q] == wc
        wi, wsc, wc = C.topk(S[q].tolist(), 10)
        assert cids[q].tolist() == wi and csc[q].tolist() == wsc and ccnt[q] == wc
    one = f["g"].retrieve(index, queries, seeds_per_query=5, top_k=10, relation_types=[0])          # one filter for every query
    assert one[0][0].tolist() == ids[0].tolist() and one[1][0].tolist() == sc[0].tolist()


# ---- the blob the typed k-hop calls share --------------------------------------------------------------------------------------------
def test_typed_k_hop_is_what_it_was_after_the_first_typed_pagerank():
    """a graph of its own: its first typed call is a k-hop (the unweighted blob), then typed PPR builds the weighted one and the
    k-hop entries get its prefix"""
    edges, masks, weights = TP.random_typed_weighted(200, 500, N_TYPES, seed=21)
    weights = [max(w, _popcount(mk)) for w, mk in zip(weights, masks)]
    g = _graph(200, edges, masks, weights)
    seeds = K.random_seeds(200, 70, 3, 5)
    filters = T.random_filters(70, N_TYPES, 6, allow_empty=True)
    want = T.levels(200, np.array(edges, np.int64), masks, seeds, filters, 3)
    before = g.neighbourhood(seeds, hops=3, relation_types=filters)
    assert np.array_equal(before, want)
    lib = g.lib
    plain, weighted = int(lib.rarc_graph_types_workspace_bytes(g.n, g.m)), int(lib.rarc_graph_types_weighted_workspace_bytes(g.n, g.m))
    assert g._typed_adj.numel() == plain and getattr(g, "_typed_adj_weighted", None) is None
    f = {"n": 200, "edges": edges, "masks": masks, "weights": weights, "g": g}
    _check(f, seeds[:9], None, [int(x) for x in filters[:9]])
    assert g._typed_adj_weighted.numel() == weighted and g._typed_adj.numel() == plain
    assert g._typed_adj.data_ptr() == g._typed_adj_weighted.data_ptr()                   # one copy of the neighbour and mask planes
    after = g.neighbourhood(seeds, hops=3, relation_types=filters)
    assert np.array_equal(after, before)
    ids, hops, cnt, hc = g.neighbourhood(seeds, hops=2, max_vertices=50, relation_types=filters)
    lv = T.levels(200, np.array(edges, np.int64), masks, seeds, filters, 2)
    assert cnt.tolist() == [min(50, int((row != T.NOT_WITHIN).sum())) for row in lv]
    # a graph whose first typed call is PPR: the k-hop calls never build a blob of their own
    g2 = _graph(200, edges, masks, weights)
    _check({**f, "g": g2}, seeds[:9], None, [int(x) for x in filters[:9]])
    assert np.array_equal(g2.neighbourhood(seeds, hops=3, relation_types=filters), want) and g2._typed_adj.data_ptr() == g2._typed_adj_weighted.data_ptr()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_python_refusals_raise_before_any_launch(hub300):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    untyped = EntityGraph(4, [(0, 1), (1, 2), (2, 3)])
    with pytest.raises(ValueError, match="without type masks"):
        untyped.personalized_pagerank([[0]], relation_types=[0])
    assert untyped._ws is None                                              # nothing was seeded
    g = _graph(4, [(0, 1), (1, 2), (2, 3)], np.array([1, 2, 1], np.uint32), None)
    for bad, match in (([32], r"\[0, 32\)"), ([[0], [1], [2]], "3 filters for 2 queries"), (np.zeros(3, np.uint32), "3 filters for 2 queries")):
        with pytest.raises(ValueError, match=match):
            g.personalized_pagerank([[0], [1]], relation_types=bad)
    assert g._ws is None and getattr(g, "_typed_adj_weighted", None) is None and g._typed_adj is None
    assert g.personalized_pagerank([[0], [1]], relation_types=None).shape == (2, 4) and getattr(g, "_typed_adj_weighted", None) is None
    assert g.personalized_pagerank([[0], [0]], relation_types=[[0], [1]], damping=0.0, max_iterations=1).tolist() == [[1.0, 0, 0, 0]] * 2
