"""Typed traversal on the GPU (csrc/khop.hip) against the restatement tests/typed_ref.py: every answer is compared
element for element — the rule is ANDs and ORs of integers, so there is no band; chunk scores are compared as float64 bits.  The
shapes are the smallest that reach each path: one to four words per vertex with a partial last word and the padded fourth lane
word of three, hubs on both sides of the degree at which a vertex is split across a workgroup and one in the largest degree
list, masks of several bits, of bit 31 and of none, filters of no bit, queries without seeds, and zero and eight hops."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import passage_ref as PS
from tests import paths_ref as P
from tests import subgraph_ref as S
from tests import typed_ref as T
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu


def _graph(n, relations, types, **kw):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, relations, types=types, **kw)


def _rows(n, relations, types=None, **kw):
    from rag_arc_amd.encapsulation.database.graph_db import RelationList

    return RelationList(n, relations, types=types, **kw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(g, n, pairs, masks, seeds, filters, hops, caps=(), **kw):
    """dense levels, then for every cap: ids, hops, counts and hop_counts -> the reference levels"""
    lv = T.levels(n, pairs, masks, seeds, filters, hops)
    got = g.neighbourhood(seeds, hops=hops, relation_types=np.asarray(filters, np.uint32), **kw)
    assert got.dtype == np.uint8 and got.shape == lv.shape
    assert np.array_equal(got, lv), np.argwhere(got != lv)[:5]
    for cap in caps:
        ids, hp, cnt, hc = g.neighbourhood(seeds, hops=hops, max_vertices=cap, relation_types=np.asarray(filters, np.uint32), **kw)
        wi, wh, wc = K.listing(lv, cap)
        assert np.array_equal(hc, K.counts(lv, hops)), cap
        assert np.array_equal(cnt, wc) and np.array_equal(ids, wi) and np.array_equal(hp, wh), cap
    return lv


@pytest.fixture(scope="module")
def rnd():
    """a random typed graph: 300 vertices, 900 relations of 4 types (duplicates and both orientations occur)"""
    n = 300
    rel, ty = T.random_typed_graph(n, 900, 4, seed=11)
    pairs, masks = T.edge_masks(rel, ty)
    return {"n": n, "rel": rel, "ty": ty, "pairs": pairs, "masks": masks, "g": _graph(n, rel, ty)}


# ---- batch sizes: W = 1, 2, 3, 4 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 64, 65, 129, 256])
def test_every_word_count_and_a_partial_last_word(rnd, nq):
    f = rnd
    assert f["g"].typed and f["g"].m == len(f["pairs"])
    seeds = K.random_seeds(f["n"], nq, 2, seed=nq)                                # (some rows have no seed)
    filters = T.random_filters(nq, 4, seed=nq + 1, allow_empty=True)
    _check(f["g"], f["n"], f["pairs"], f["masks"], seeds, filters, 3, caps=(7, 300))


@pytest.mark.parametrize("hops", [0, 1, 8])
def test_zero_and_eight_hops(rnd, hops):
    f = rnd
    seeds = K.random_seeds(f["n"], 70, 1, seed=3)
    _check(f["g"], f["n"], f["pairs"], f["masks"], seeds, T.random_filters(70, 4, seed=4), hops, caps=(40,), early_stop=bool(hops == 8))


# ---- degrees: the group / split boundary, and the largest degree list ---------------------------------------------------------------------
def _star(leaves):
    """hub 0, leaf i joined by a relation of type i % 3, every fifth leaf by a second one of type 3 (swapped: a two-bit mask); a
    tail n behind the last leaf, type 0 -> (n + 1, relations, types)"""
    n, edges = K.star_graph(leaves)
    rel, ty = [list(e) for e in edges], [i % 3 for i in range(1, leaves + 1)]
    for i in range(5, leaves + 1, 5):
        rel.append([i, 0])
        ty.append(3)
    rel.append([leaves, n])
    ty.append(0)
    return n + 1, np.array(rel, np.int64), np.array(ty, np.int64)


@pytest.mark.parametrize("leaves,nq", [(1, 3), (8, 70), (64, 70), (65, 70), (65, 200), (8193, 70), (8193, 130)])
def test_a_hub_on_both_sides_of_the_split_and_in_the_largest_degree_list(leaves, nq):
    n, rel, ty = _star(leaves)
    pairs, masks = T.edge_masks(rel, ty)
    g = _graph(n, rel, ty)
    rng = np.random.default_rng(leaves + nq)
    seeds = [[int(rng.integers(1, leaves + 1))] for _ in range(nq)]                # a leaf each: the hub joins what differs per wave
    seeds[0], seeds[-1] = [0], [n - 1]
    if nq > 2:
        seeds[1] = []
    filters = T.random_filters(nq, 4, seed=leaves, allow_empty=True)
    filters[-1] = T.ALL
    for hops in (1, 3):
        lv = _check(g, n, pairs, masks, seeds, filters, hops, caps=(min(n, 100),))
    assert lv[-1, 0] == 2 and lv[-1, 1] == (3 if leaves > 1 else 1)                # tail -> last leaf -> hub -> every leaf


# ---- mask cases ---------------------------------------------------------------------------------------------------------------------------
def test_the_mask_cases_the_rule_names():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    # 0 -{1}- 1 -{0}- 2, 0 -{0, 1}- 3, 3 -{31}- 4, and the pair (2, 3) of mask 0 (device pairs: a mask need not be non-zero)
    pairs = np.array([[0, 1], [0, 3], [1, 2], [2, 3], [3, 4]], np.int64)
    masks = np.array([2, 3, 1, 0, 1 << 31], np.uint32)
    g = EntityGraph.from_device(5, torch.from_numpy(pairs).cuda(), type_masks=torch.from_numpy(masks.view(np.int32)).cuda())
    assert g.typed
    seeds = [[0], [0], [0], [0], [], [3], [4]]
    filters = np.array([1, 2, 0, T.ALL, T.ALL, T.ALL, 1 << 31], np.uint32)
    for hops in (0, 1, 3, 8):
        lv = _check(g, 5, pairs, masks, seeds, filters, hops, caps=(1, 5))
    assert lv[0].tolist() == [0, 255, 255, 1, 255]                                 # {0, 1} crossed on type 0 alone ..
    assert lv[1].tolist() == [0, 1, 255, 1, 255]                                   # .. and on type 1 alone
    assert lv[2].tolist() == [0, 255, 255, 255, 255] and lv[4].tolist() == [255] * 5   # F = 0: the seed alone; no seed: nothing
    assert lv[5].tolist() == [1, 2, 3, 0, 1]                                       # the mask-0 pair (2, 3): one hop untyped, three typed
    assert g.neighbourhood([[3]], hops=3)[0].tolist() == [1, 2, 1, 0, 1]
    assert lv[6].tolist() == [255, 255, 255, 1, 0]                                 # type 31
    # the filter forms agree: ids, per-query ids, masks
    a = g.neighbourhood(seeds[:2], hops=3, relation_types=[[0], [1]])
    assert np.array_equal(a, lv[:2]) and np.array_equal(g.neighbourhood(seeds[:1], hops=3, relation_types=[0]), lv[:1])


def test_refusals_on_a_device():
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    g = EntityGraph(3, [(0, 1), (1, 2)])
    assert not g.typed
    with pytest.raises(ValueError, match="without type masks"):
        g.neighbourhood([[0]], relation_types=[0])
    t = _graph(3, [(0, 1), (1, 2)], [0, 1])
    with pytest.raises(ValueError, match="2 filters for 3 queries"):
        t.neighbourhood([[0], [1], [2]], relation_types=[[0], [1]])
    with pytest.raises(ValueError, match="RelationList without types"):
        t.subgraph([[0]], relations=_rows(3, [(0, 1)]), relation_types=[0])
    with pytest.raises(ValueError, match="paths call"):
        t.shortest_paths([[0], [2]], [(0, 1)], relation_types=[[0], [1]])
    assert t._typed_adj is None                                                    # nothing was built for a refused call


def test_a_pair_list_that_is_not_the_graphs_is_reported():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph
    from rag_arc_amd.hip import binding as B

    g = EntityGraph(6, K.path_graph(6))
    other = torch.tensor([[0, 1], [0, 2], [0, 3], [0, 4], [0, 5]], dtype=torch.int64).cuda()     # vertex 0 has one slot, not five
    masks = torch.ones(5, dtype=torch.int32).cuda()
    out = torch.empty(int(g.lib.rarc_graph_types_workspace_bytes(6, 5)), dtype=torch.uint8).cuda()
    rc = g.lib.rarc_graph_types(g._graph.data_ptr(), g._graph.numel(), 6, 5, other.data_ptr(), masks.data_ptr(), out.data_ptr(), out.numel(), None)
    assert rc == -1 and b"4 pairs found their rows full" in B.load_library().rarc_last_error()


# ---- reduction and order independence ---------------------------------------------------------------------------------------------------
def test_all_ones_filters_are_the_untyped_answers_bit_for_bit(rnd):
    f, g = rnd, rnd["g"]
    assert f["masks"].min() > 0
    seeds = K.random_seeds(f["n"], 130, 2, seed=21)
    ones = np.full(130, T.ALL, np.uint32)
    mentions, weights = PS.random_mentions(f["n"], 40, seed=22, max_degree=8, max_weight=9)
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    mm = MentionMap(40, f["n"], mentions, weights=weights)
    rel = _rows(f["n"], f["rel"], f["ty"])
    for hops in (1, 3):
        assert np.array_equal(g.neighbourhood(seeds, hops=hops, relation_types=ones), g.neighbourhood(seeds, hops=hops))
        for a, b in zip(g.neighbourhood(seeds, hops=hops, max_vertices=33, relation_types=ones), g.neighbourhood(seeds, hops=hops, max_vertices=33)):
            assert np.array_equal(a, b)
        assert np.array_equal(_bits(g.neighbourhood_chunks(mm, seeds, hops=hops, relation_types=ones)), _bits(g.neighbourhood_chunks(mm, seeds, hops=hops)))
        for relations in (None, rel):
            typed = g.subgraph(seeds, hops=hops, max_vertices=50, max_edges=60, relations=relations, relation_types=ones)
            plain = g.subgraph(seeds, hops=hops, max_vertices=50, max_edges=60, relations=relations)
            for a, b in zip(typed, plain):
                assert (a is None and b is None) or np.array_equal(a, b)


def test_the_answer_does_not_depend_on_the_order_of_pairs_or_queries(rnd):
    f = rnd
    seeds = K.random_seeds(f["n"], 90, 2, seed=31)
    filters = T.random_filters(90, 4, seed=32)
    want = f["g"].neighbourhood(seeds, hops=3, relation_types=filters)
    order = np.random.default_rng(33).permutation(len(f["rel"]))
    g2 = _graph(f["n"], f["rel"][order][:, ::-1], f["ty"][order])
    assert np.array_equal(g2.neighbourhood(seeds, hops=3, relation_types=filters), want)
    qo = np.random.default_rng(34).permutation(90)
    assert np.array_equal(f["g"].neighbourhood([seeds[q] for q in qo], hops=3, relation_types=filters[qo]), want[qo])
    for q in (0, 63, 64, 89):                                                      # row q of a batch is the one-query call
        assert np.array_equal(f["g"].neighbourhood([seeds[q]], hops=3, relation_types=filters[q:q + 1])[0], want[q])


def test_one_filter_is_b_copies_of_it_and_batches_above_256_are_cut_with_their_filters(rnd):
    f, g = rnd, rnd["g"]
    seeds = K.random_seeds(f["n"], 70, 2, seed=41)
    one = g.neighbourhood(seeds, hops=2, relation_types=[1, 3])
    assert np.array_equal(one, g.neighbourhood(seeds, hops=2, relation_types=[[1, 3]] * 70))
    assert np.array_equal(one, T.levels(f["n"], f["pairs"], f["masks"], seeds, [0b1010] * 70, 2))
    many = K.random_seeds(f["n"], 300, 1, seed=42)
    filters = T.random_filters(300, 4, seed=43)
    assert np.array_equal(g.neighbourhood(many, hops=2, relation_types=filters), T.levels(f["n"], f["pairs"], f["masks"], many, filters, 2))


# ---- typed rows ---------------------------------------------------------------------------------------------------------------------------
def test_rows_are_listed_for_the_queries_that_allow_their_type(rnd):
    f, g = rnd, rnd["g"]
    # a small case by hand: two rows of different types over one pair, a refused row inside the neighbourhood
    t = _graph(4, [(0, 1), (1, 0), (1, 2), (2, 3)], [0, 1, 0, 1])
    rel = _rows(4, [(0, 1), (1, 0), (1, 2), (2, 3), (0, 2), (3, 3)], [0, 1, 0, 1, 1, 0])
    got = t.subgraph([[0], [0], [0]], hops=2, relations=rel, relation_types=[[0], [1], [0, 1]])
    assert [got.edge_ids[q, :got.edge_counts[q]].tolist() for q in range(3)] == [[0, 2], [1], [0, 1, 2, 4]]
    plain = t.subgraph([[0]], hops=2, relations=rel)
    assert plain.edge_ids[0, :plain.edge_counts[0]].tolist() == [0, 1, 2, 4]       # (0, 2) joins two vertices query 0 reaches: refused by type
    assert got.edge_level_counts.tolist() == [[0, 1, 1], [0, 1, 0], [0, 2, 2]]
    # random: the caller's typed table, more than one tile of rows, two words of queries, cuts
    rows = S.typed_relations(f["pairs"], seed=51, repeats=2)
    rt = np.random.default_rng(52).integers(0, 5, size=len(rows))                  # (type 4 is in no filter below)
    rl = _rows(f["n"], rows, rt)
    assert rl.typed and len(rows) > 1024
    seeds = K.random_seeds(f["n"], 70, 2, seed=53)
    filters = T.random_filters(70, 4, seed=54, allow_empty=True)
    for hops, cap in ((2, 9), (3, 4000)):
        wi, wl, wc, wlc = T.subgraph(f["n"], f["pairs"], f["masks"], seeds, filters, hops, rows, T.type_bits(rt), cap)
        for got in (g.subgraph(seeds, hops=hops, max_edges=cap, relations=rl, relation_types=filters),
                    g.neighbourhood_edges(seeds, hops=hops, max_edges=cap, relations=rl, relation_types=filters)):
            assert np.array_equal(got.edge_level_counts, wlc) and np.array_equal(got.edge_counts, wc)
            assert np.array_equal(got.edge_ids, wi) and np.array_equal(got.edge_levels, wl)
        # the graph's own pairs: a pair is listed iff its mask shares a type with the filter
        wi, wl, wc, wlc = T.subgraph(f["n"], f["pairs"], f["masks"], seeds, filters, hops, f["pairs"], f["masks"], cap)
        got = g.neighbourhood_edges(seeds, hops=hops, max_edges=cap, relation_types=filters)
        assert np.array_equal(got.edge_level_counts, wlc) and np.array_equal(got.edge_ids, wi) and np.array_equal(got.edge_levels, wl)


# ---- typed paths --------------------------------------------------------------------------------------------------------------------------
def test_paths_under_a_filter():
    # a 6-cycle whose edge (0, 5) has type 1 and the others type 0, and a pendant 6 behind 0 by type 1
    rel = np.array(P.cycle_graph(6) + [(0, 6)], np.int64)
    ty = np.array([0, 0, 0, 0, 0, 1, 1], np.int64)
    pairs, masks = T.edge_masks(rel, ty)
    g = _graph(7, rel, ty)
    rows = _rows(7, rel, ty)
    sources, sp = [[0], [5], [6], [2]], [(0, 1), (0, 2), (1, 3), (2, 2)]
    for f in (0b01, 0b10, 0b11):
        d, pos = T.paths(7, pairs, masks, sources, sp, f, 6)
        got = g.shortest_paths(sources, sp, max_length=6, max_vertices=7, max_edges=7, relations=rows, relation_types=T_ids(f))
        assert np.array_equal(got.distances, d)
        wi, wp, wc = P.listing(pos, 7)
        assert np.array_equal(got.vertex_ids, wi) and np.array_equal(got.vertex_positions, wp) and np.array_equal(got.vertex_counts, wc)
        rl = T.path_row_levels(pos, rel, T.type_bits(ty), f)
        ei, el, ec = P.listing(rl, 7)
        assert np.array_equal(got.edge_ids, ei) and np.array_equal(got.edge_levels, el) and np.array_equal(got.edge_counts, ec)
        assert np.array_equal(got.edge_level_counts, P.counts(rl, 6))
        own = g.shortest_paths(sources, sp, max_length=6, max_vertices=7, max_edges=7, relation_types=T_ids(f))
        ol = T.path_row_levels(pos, pairs, masks, f)
        assert np.array_equal(own.edge_ids, P.listing(ol, 7)[0]) and np.array_equal(own.distances, d)
    d0, _ = T.paths(7, pairs, masks, sources, sp, 0b01, 6)
    assert d0.tolist() == [5, -1, 3, 0]                                            # 0 .. 5 the long way round; 6 is cut off; 6 - 6 is a source
    untyped = g.shortest_paths(sources, sp, max_length=6)
    assert untyped.distances.tolist() == [1, 1, 3, 0]


def T_ids(f):
    return [t for t in range(32) if (f >> t) & 1]


# ---- chunks and the retriever ---------------------------------------------------------------------------------------------------------------
def test_chunks_are_the_references_integer_sums(rnd):
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    f, g = rnd, rnd["g"]
    mentions, weights = PS.random_mentions(f["n"], 50, seed=61, max_degree=70, max_weight=9)
    mm = MentionMap(50, f["n"], mentions, weights=weights)
    seeds = K.random_seeds(f["n"], 66, 2, seed=62)
    filters = T.random_filters(66, 4, seed=63, allow_empty=True)
    lv = T.levels(f["n"], f["pairs"], f["masks"], seeds, filters, 2)
    want = K.chunk_scores(lv, 50, mentions, weights, K.default_decay(2))
    assert np.array_equal(_bits(g.neighbourhood_chunks(mm, seeds, hops=2, relation_types=filters)), _bits(want))
    ids, sc, cnt = g.neighbourhood_chunks(mm, seeds, hops=2, top_k=5, relation_types=filters)
    for q in range(66):
        wi, ws, wc = K.chunk_topk([int(x) for x in np.rint(want[q] * K.SCORE_ONE)], 5)
        assert cnt[q] == wc and ids[q].tolist() == wi and _bits(sc[q]).tolist() == _bits(ws).tolist(), q


def test_the_retriever_with_one_filter_per_query():
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    n_ent, n_chunks, dim = 500, 80, 64
    emb = HashEmbeddings(dim)
    x = np.asarray(emb.embed_documents([f"entity {i}" for i in range(n_ent)]), np.float32)
    rel, ty = T.random_typed_graph(n_ent, 1500, 3, seed=71)
    mentions, weights = PS.random_mentions(n_ent, n_chunks, seed=72, max_degree=8, max_weight=9)
    texts, ids = [f"chunk {i}" for i in range(n_chunks)], [f"c{i}" for i in range(n_chunks)]
    r = HipGraphRetriever.from_arrays(emb, x, rel, mentions, texts, mention_weights=weights, ids=ids, k=6, expansion="k_hop", hops=2,
                                      pair_types=ty, relation_types=[0])
    queries = ["entity 3", "entity 417", "who founded entity 5", "entity 499"]
    filters = [[0], [1, 2], [], [0, 1, 2]]
    batch = r.batch_invoke(queries, relation_types=filters)
    for q, fl, docs in zip(queries, filters, batch):
        alone = r.invoke(q, relation_types=fl)
        assert [(d.id, d.score) for d in alone] == [(d.id, d.score) for d in docs]
    assert [(d.id, d.score) for d in r.invoke(queries[0])] == [(d.id, d.score) for d in batch[0]]      # the constructor's filter
    assert [d.id for d in batch[1]] != [d.id for d in batch[3]] or [d.score for d in batch[1]] != [d.score for d in batch[3]]
    with pytest.raises(ValueError, match="typed personalized PageRank is not built"):
        HipGraphRetriever(emb, r.index, r.graph, r.mentions, r.docs, relation_types=[0])


def test_from_relations_builds_pairs_masks_and_weights():
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    rel = [(0, 1), (1, 0), (1, 2), (2, 2), (0, 1), (3, 7)]
    ty = [0, 5, 1, 3, 0, 0]
    g = EntityGraph.from_relations(_rows(4, rel, ty))                              # (2, 2) and (3, 7) are no edges of a graph on 4 vertices
    assert g.typed and g._pairs.cpu().tolist() == [[0, 1], [1, 2]]
    assert g._type_masks.cpu().numpy().view(np.uint32).tolist() == [0b100001, 0b10] and g._pair_weights.cpu().tolist() == [3, 1]
    gw = EntityGraph.from_relations(_rows(4, rel, ty, weights=[2, 3, 4, 5, 6, 7]))
    assert gw._pair_weights.cpu().tolist() == [11, 4]
    assert g.neighbourhood([[0]], hops=2, relation_types=[5])[0].tolist() == [0, 1, 255, 255]
