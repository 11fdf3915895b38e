"""tests/typed_ref.py, the specification of the typed traversal, against an independent brute force, and the host
side of the feature: mask ORing in EntityGraph's normalisation, type names, and every refusal that needs no device."""
import types as pytypes

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import shortest_path

from rag_arc_amd.encapsulation.database.graph_db import RelationList, k_hop, k_hop_subgraph, shortest_paths
from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as NB
from rag_arc_amd.encapsulation.database.graph_db import pagerank as PR
from rag_arc_amd.hip import binding as B
from tests import khop_ref as K
from tests import paths_ref as P
from tests import subgraph_ref as S
from tests import typed_ref as T


def brute_levels(n, pairs, masks, seed_lists, filters, hops):
    """per query: scipy's unweighted shortest paths on the graph of the edges the filter crosses, from every seed"""
    out = np.full((len(seed_lists), n), T.NOT_WITHIN, np.uint8)
    for q, (seeds, f) in enumerate(zip(seed_lists, filters)):
        seeds = sorted({int(v) for v in seeds if 0 <= int(v) < n})
        if not seeds:
            continue
        keep = (np.asarray(masks, np.uint32) & np.uint32(f)) != 0
        e = np.asarray(pairs, np.int64).reshape(-1, 2)[keep]
        g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()
        d = shortest_path(g, method="D", directed=False, unweighted=True, indices=seeds).min(axis=0)
        inside = d <= hops
        out[q, inside] = d[inside].astype(np.uint8)
    return out


@pytest.mark.parametrize("n,m,n_types,hops,seed", [(40, 60, 1, 3, 0), (120, 200, 3, 4, 1), (200, 500, 5, 2, 2), (200, 260, 4, 8, 3),
                                                    (7, 30, 2, 0, 4)])
def test_the_reference_equals_a_per_query_bfs_of_the_filtered_graph(n, m, n_types, hops, seed):
    rel, ty = T.random_typed_graph(n, m, n_types, seed)
    pairs, masks = T.edge_masks(rel, ty)
    seeds = K.random_seeds(n, 23, 3, seed + 10)
    filters = T.random_filters(23, n_types, seed + 20, allow_empty=True)
    want = brute_levels(n, pairs, masks, seeds, filters, hops)
    got = T.levels(n, pairs, masks, seeds, filters, hops)
    assert np.array_equal(got, want)
    for q in (0, 4, 22):
        assert np.array_equal(T.levels_one(n, pairs, masks, seeds[q], filters[q], hops), want[q])


def test_all_ones_filters_over_non_zero_masks_are_the_untyped_rule():
    rel, ty = T.random_typed_graph(150, 300, 5, 7)
    pairs, masks = T.edge_masks(rel, ty)
    assert masks.min() > 0
    seeds = K.random_seeds(150, 17, 4, 8)
    for hops in (0, 1, 3, 8):
        lv = T.levels(150, pairs, masks, seeds, [T.ALL] * 17, hops)
        assert np.array_equal(lv, K.levels(150, pairs, seeds, hops))
        rows = T.row_levels(lv, rel, T.type_bits(ty), [T.ALL] * 17)
        assert np.array_equal(rows, S.row_levels(lv, rel))
    d, pos = T.paths(150, pairs, masks, seeds, [(0, 1), (2, 3), (5, 5)], T.ALL, 6)
    wd, wpos = P.paths(150, pairs, seeds, [(0, 1), (2, 3), (5, 5)], 6)
    assert np.array_equal(d, wd) and np.array_equal(pos, wpos)


def test_the_consequences_the_rule_names():
    # 0 -1- 1 -0- 2, and 0 -{0,1}- 3; the pair (2, 3) has mask 0
    pairs, masks = np.array([[0, 1], [0, 3], [1, 2], [2, 3]]), np.array([2, 3, 1, 0], np.uint32)
    lv = T.levels(4, pairs, masks, [[0], [0], [0], [0], []], [1, 2, 0, T.ALL, T.ALL], 3)
    assert lv.tolist() == [[0, 255, 255, 1], [0, 1, 255, 1], [0, 255, 255, 255], [0, 1, 2, 1], [255] * 4]
    # a mask-0 edge is crossed by nobody: 3 -> 2 only through 0 - 1 - 2 under all ones
    assert T.levels(4, pairs, masks, [[3]], [T.ALL], 3)[0].tolist() == [1, 2, 3, 0]
    # typed rows: two rows of different types over one pair, one with a type outside [0, 32), one with an end outside [0, n)
    rel, ty = [(0, 3), (3, 0), (0, 3), (0, 4)], [0, 1, 32, 0]
    rl = T.row_levels(lv[:2], rel, T.type_bits(ty), [1, 2])
    assert rl.tolist() == [[1, 255, 255, 255], [255, 1, 255, 255]]
    assert T.type_bits([0, 31, 32, -1]).tolist() == [1, 1 << 31, 0, 0]


def test_masks_are_ored_over_duplicate_and_swapped_input_pairs():
    pairs = [(0, 1), (1, 0), (0, 1), (2, 1), (1, 2), (3, 0)]
    ty = [0, 4, 0, 31, 2, 7]
    want_pairs, want_masks = T.edge_masks(pairs, ty)
    assert want_pairs.tolist() == [[0, 1], [0, 3], [1, 2]] and want_masks.tolist() == [0b10001, 1 << 7, (1 << 31) | 4]
    arr, w, masks = PR._normalise_typed_pairs(4, pairs, None, ty)
    assert np.array_equal(arr, want_pairs) and w is None and masks.dtype == np.uint32 and np.array_equal(masks, want_masks)
    arr, w, masks = PR._normalise_typed_pairs(4, pairs, [1, 2, 3, 4, 5, 6], ty)
    assert w.tolist() == [6, 6, 9] and np.array_equal(masks, want_masks)
    # without types nothing changes, and the two-value form the other modules import is what it was
    arr2, w2 = PR._normalise_pairs(4, pairs, [1, 2, 3, 4, 5, 6])
    assert np.array_equal(arr2, arr) and np.array_equal(w2, w)
    assert PR._normalise_typed_pairs(4, pairs, None, None)[2] is None
    rel, rt = T.random_typed_graph(50, 400, 6, 5)
    wp, wm = T.edge_masks(rel, rt)
    assert len(wp) < 400                                                           # (duplicates occurred)
    order = np.random.default_rng(5).permutation(400)
    for r, t in ((rel, rt), (rel[order], rt[order]), (rel[:, ::-1], rt)):
        arr, _, masks = PR._normalise_typed_pairs(50, r, None, t)
        assert np.array_equal(arr, wp) and np.array_equal(masks, wm)


def test_type_ids_and_the_limit_of_32_types():
    ids, vocab = RelationList.type_ids(["causal", "sequential", "causal", "conditional", "sequential"])
    assert ids.tolist() == [0, 1, 0, 2, 1] and ids.dtype == np.int32 and vocab == ["causal", "sequential", "conditional"]
    ids, vocab = RelationList.type_ids([f"t{i % 32}" for i in range(100)])
    assert ids.max() == 31 and len(vocab) == 32
    with pytest.raises(B.RarcUnsupported, match="32"):
        RelationList.type_ids([f"t{i}" for i in range(33)])
    assert RelationList.type_ids([])[1] == []


def test_filters_in_every_form():
    assert NB.host_filters([0, 3]).tolist() == [9] and NB.host_filters([31]).tolist() == [1 << 31] and NB.host_filters([]).tolist() == [0]
    assert NB.host_filters([[0], [1, 2], []]).tolist() == [1, 6, 0]
    assert NB.host_filters((x for x in [{0, 1}, (5,)])).tolist() == [3, 32]
    masks = np.array([1, 0xFFFFFFFF, 0], np.uint32)
    assert NB.host_filters(masks) is masks or np.array_equal(NB.host_filters(masks), masks)
    assert NB.host_filters(np.array([2, 3], np.int64)).tolist() == [12]               # (an int array is a list of ids, not of masks)
    assert NB.spread_filters(np.array([5], np.uint32), 4).tolist() == [5] * 4
    assert NB.spread_filters(np.array([5, 6], np.uint32), 2).tolist() == [5, 6]
    for bad in ([32], [-1], [0.5], [True], ["causal"], [[0], [32]], [0, [1]], 3, "causal", np.zeros((2, 2), np.uint32), np.zeros(0, np.uint32)):
        with pytest.raises(ValueError):
            NB.host_filters(bad)
    for count in (2, 3, 5):
        with pytest.raises(ValueError, match="one filter for all of them or one per query"):
            NB.spread_filters(np.zeros(count, np.uint32), 4)


def test_every_refusal_that_needs_no_device():
    pairs = [(0, 1), (1, 2)]
    untyped = pytypes.SimpleNamespace(typed=False)
    typed = pytypes.SimpleNamespace(typed=True)
    assert NB.check_typed(untyped, None) is None and NB.check_typed(typed, None) is None
    with pytest.raises(ValueError, match="without type masks"):
        NB.check_typed(untyped, [0])
    with pytest.raises(ValueError, match=r"\[0, 32\)"):
        NB.check_typed(typed, [32])
    assert NB.check_typed(typed, [[0], [1]]).tolist() == [1, 2]
    # paths take one filter
    with pytest.raises(ValueError, match="paths call"):
        NB._single_filter(typed, [[0], [1]])
    assert NB._single_filter(typed, [0, 1]).tolist() == [3] and NB._single_filter(typed, None) is None
    # the one-shot forms, before a graph is built
    with pytest.raises(ValueError, match="without type masks"):
        k_hop(3, pairs, [[0]], relation_types=[0])
    with pytest.raises(ValueError, match=r"\[0, 32\)"):
        k_hop(3, pairs, [[0]], types=[0, 1], relation_types=[40])
    with pytest.raises(ValueError, match="3 filters for 2 queries"):
        k_hop(3, pairs, [[0], [1]], types=[0, 1], relation_types=[[0], [1], [0]])
    with pytest.raises(ValueError, match="3 filters for 1 queries"):
        k_hop_subgraph(3, pairs, [[0]], types=[0, 1], relation_types=[[0], [1], [0]])
    with pytest.raises(ValueError, match="paths call"):
        shortest_paths(3, pairs, [[0], [2]], [(0, 1)], types=[0, 1], relation_types=[[0], [1]])
    # the types of a graph and of a relation list
    for bad in ([0], [0, 32], [0, -1], [0, 0.5], [[0, 1]]):
        with pytest.raises(ValueError, match="type"):
            k_hop(3, pairs, [[0]], types=bad)
        with pytest.raises(ValueError, match="type"):
            RelationList(3, pairs, types=bad)
    # a typed subgraph needs a typed relation list
    rel = RelationList.__new__(RelationList)
    rel.n_entities, rel.device = 3, "cuda:0"
    graph = pytypes.SimpleNamespace(n=3, device="cuda:0")
    NB.check_relations(graph, rel)
    NB.check_relations(graph, None, typed=True)
    with pytest.raises(ValueError, match="RelationList without types"):
        NB.check_relations(graph, rel, typed=True)
    rel._types = object()
    NB.check_relations(graph, rel, typed=True)
    with pytest.raises(ValueError, match="RelationList with types"):
        PR.EntityGraph.from_relations(RelationList.__new__(RelationList))


def test_the_retriever_refuses_typed_pagerank_and_untyped_graphs():
    from rag_arc_amd.core.retrieval.graph import HipGraphRetriever as R

    typed = pytypes.SimpleNamespace(typed=True)
    R._check_relation_types("ppr", typed, None)
    R._check_relation_types("k_hop", typed, [0, 1])
    with pytest.raises(ValueError, match="typed personalized PageRank is not built"):
        R._check_relation_types("ppr", typed, [0])
    with pytest.raises(ValueError, match="without type masks"):
        R._check_relation_types("k_hop", pytypes.SimpleNamespace(typed=False), [0])
    with pytest.raises(ValueError, match="pair_types without pairs"):
        R.from_arrays(None, np.zeros((3, 4), np.float32), pairs=None, mentions=[(0, 0)], texts=["a"], pair_types=[0])
