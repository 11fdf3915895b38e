"""The k-hop reference (tests/khop_ref.py) against networkx and against itself: what the GPU tests compare with must be right
before it is a yardstick."""
import numpy as np
import pytest

from tests import khop_ref as K


@pytest.mark.parametrize("n,m,seed", [(30, 40, 1), (200, 300, 2), (500, 2000, 3)])
def test_levels_equal_networkx_shortest_path_lengths(n, m, seed):
    nx = pytest.importorskip("networkx")
    edges, _ = K.random_graph(n, m, seed)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    for hops in (0, 1, 3, 8):
        for s in (0, n // 2, n - 1):
            want = np.full(n, K.NOT_WITHIN, np.uint8)
            for v, d in nx.single_source_shortest_path_length(g, s, cutoff=hops).items():
                want[v] = d
            assert np.array_equal(K.levels_one(n, edges, [s], hops), want)


def test_multi_seed_is_the_minimum_over_single_seeds():
    n = 300
    edges, _ = K.random_graph(n, 500, 4)
    for hops in (0, 2, 5):
        for seeds in ([3], [3, 3, 250], [0, 17, 99, 299], [], [-1, 5, -1]):
            singles = [K.levels_one(n, edges, [s], hops) for s in seeds if s >= 0]
            want = np.min(np.stack(singles), axis=0) if singles else np.full(n, K.NOT_WITHIN, np.uint8)
            assert np.array_equal(K.levels_one(n, edges, seeds, hops), want)


def test_the_batched_forms_equal_the_plain_ones():
    from tests import passage_ref as P

    n, n_chunks = 300, 120
    edges, _ = K.random_graph(n, 450, 7)
    seeds = K.random_seeds(n, 9, 4, 8) + [[], [-1, -1], [5, 5, n, -7]]
    mentions, weights = P.random_mentions(n, n_chunks, seed=9, max_degree=6, max_weight=40)
    mentions, weights = mentions + mentions[:10], weights + weights[:10]          # (duplicates: their weights add up)
    for hops in (0, 1, 4, 8):
        lv = K.levels(n, edges, seeds, hops)
        assert np.array_equal(lv, np.stack([K.levels_one(n, edges, s, hops) for s in seeds]))
        for decay in (K.default_decay(hops), [7] + [0] * hops, [65536] * (hops + 1)):
            want = [[x / K.SCORE_ONE for x in K.chunk_state(row, n_chunks, mentions, weights, decay)] for row in lv]
            assert np.array_equal(K.chunk_scores(lv, n_chunks, mentions, weights, decay), np.array(want))
    assert np.array_equal(K.levels(4, [], [[1]], 3), [[255, 0, 255, 255]])


def test_counts_add_up_to_the_list_length_when_uncapped_and_the_cap_cuts_in_order():
    n = 400
    edges, _ = K.random_graph(n, 900, 5)
    seeds = K.random_seeds(n, 7, 3, 6) + [[]]
    lv = K.levels(n, edges, seeds, 3)
    cnt = K.counts(lv, 3)
    ids, hp, c = K.listing(lv, n)
    assert np.array_equal(cnt.sum(axis=1), c) and c[-1] == 0 and c[:-1].min() > 0
    for q in range(len(seeds)):
        assert np.array_equal(hp[q, :c[q]], lv[q][ids[q, :c[q]]]) and np.all(ids[q, c[q]:] == -1) and np.all(hp[q, c[q]:] == -1)
        keys = list(zip(hp[q, :c[q]].tolist(), ids[q, :c[q]].tolist()))
        assert keys == sorted(keys) and len(set(ids[q, :c[q]].tolist())) == c[q]
        ids2, hp2, c2 = K.listing(lv[q:q + 1], 5)
        assert c2[0] == min(5, c[q]) and np.array_equal(ids2[0, :c2[0]], ids[q, :c2[0]]) and np.array_equal(hp2[0, :c2[0]], hp[q, :c2[0]])


def test_hops_zero_is_the_distinct_seeds():
    lv = K.levels(20, K.path_graph(20), [[4, 4, 9]], 0)
    ids, hp, c = K.listing(lv, 8)
    assert ids[0, :2].tolist() == [4, 9] and c[0] == 2 and K.counts(lv, 0).tolist() == [[2]]


def test_chunk_scores_weigh_a_mention_by_the_decay_of_its_hop():
    edges = K.path_graph(6)
    lv = K.levels(6, edges, [[0]], 2)
    mentions, weights = [(0, 0), (0, 2), (1, 3), (2, 1), (2, 1)], [3, 5, 7, 2, 4]
    assert K.chunk_state(lv[0], 4, mentions, weights, K.default_decay(2)) == [3 * 4096 + 5 * 256, 0, 6 * 1024, 0]
    assert K.chunk_state(lv[0], 4, mentions, weights, [1, 0, 65536]) == [3 + 5 * 65536, 0, 0, 0]
    assert K.default_decay(8) == [4096, 1024, 256, 64, 16, 4, 1, 0, 0]
