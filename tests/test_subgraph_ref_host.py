"""The k-hop subgraph reference (tests/subgraph_ref.py) against a brute-force loop over networkx and against itself: what the
GPU tests compare with must be right before it is a yardstick."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import subgraph_ref as S


def _brute(dist, relations, hops, n):
    """one query: [(level, row)] sorted, from a {vertex: distance} map — the definition, row by row"""
    out = []
    for e, (a, b) in enumerate(relations):
        if 0 <= a < n and 0 <= b < n and a in dist and b in dist and max(dist[a], dist[b]) <= hops:
            out.append((max(dist[a], dist[b]), e))
    return sorted(out)


@pytest.mark.parametrize("n,m,seed", [(30, 40, 1), (200, 300, 2), (500, 2000, 3)])
def test_the_reference_equals_a_loop_over_networkx_shortest_path_lengths(n, m, seed):
    nx = pytest.importorskip("networkx")
    edges, _ = K.random_graph(n, m, seed)
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    rel = S.typed_relations(edges, seed + 10, repeats=2).tolist() + [[3, 3], [-1, 0], [0, n], [n - 1, 0]]
    seeds = [[0], [n // 2, n - 1], [], [5, 5, 6]]
    for hops in (0, 1, 3, 8):
        ids, lv, cnt, lc = S.subgraph(n, edges, seeds, hops, rel, len(rel))
        for q, s in enumerate(seeds):
            dist = {}
            for v in s:
                for u, d in nx.single_source_shortest_path_length(g, v, cutoff=hops).items():
                    dist[u] = min(d, dist.get(u, d))
            want = _brute(dist, rel, hops, n)
            assert list(zip(lv[q, :cnt[q]].tolist(), ids[q, :cnt[q]].tolist())) == want and cnt[q] == len(want)
            assert lc[q].tolist() == [sum(1 for l, _ in want if l == h) for h in range(hops + 1)]


def test_the_reference_equals_the_definition_without_networkx_and_the_bit_form_the_kernel_evaluates():
    n = 300
    edges, _ = K.random_graph(n, 500, 4)
    rel = S.typed_relations(edges, 5).tolist() + [[7, 7], [n, 1], [1, -1]]
    seeds = K.random_seeds(n, 6, 3, 6) + [[]]
    for hops in (0, 2, 5):
        dense = K.levels(n, edges, seeds, hops)
        rl = S.row_levels(dense, rel)
        bits = S.level_bits(dense, rel, hops)
        ids, lv, cnt, lc = S.subgraph(n, edges, seeds, hops, rel, len(rel))
        for q, s in enumerate(seeds):
            one = K.levels_one(n, edges, s, hops)
            dist = {v: int(one[v]) for v in range(n) if one[v] != K.NOT_WITHIN}
            want = _brute(dist, rel, hops, n)
            assert list(zip(lv[q, :cnt[q]].tolist(), ids[q, :cnt[q]].tolist())) == want
            for h in range(hops + 1):
                assert np.array_equal(bits[h, q], rl[q] == h)
        assert np.array_equal(bits.sum(axis=2).T, lc)


def test_level_counts_equal_the_list_length_when_uncapped_and_the_cap_cuts_in_order():
    n = 400
    edges, _ = K.random_graph(n, 900, 5)
    rel = S.typed_relations(edges, 6)
    seeds = K.random_seeds(n, 7, 3, 6) + [[]]
    ids, lv, cnt, lc = S.subgraph(n, edges, seeds, 3, rel, len(rel))
    assert np.array_equal(lc.sum(axis=1), cnt) and cnt[-1] == 0 and (cnt > 0).sum() >= 5      # (random_seeds leaves some rows empty)
    for q in range(len(seeds)):
        keys = list(zip(lv[q, :cnt[q]].tolist(), ids[q, :cnt[q]].tolist()))
        assert keys == sorted(keys) and len(set(ids[q, :cnt[q]].tolist())) == cnt[q]
        assert np.all(ids[q, cnt[q]:] == -1) and np.all(lv[q, cnt[q]:] == -1)
        for cap in (1, 5, max(int(cnt[q]) - 1, 1)):
            ids2, lv2, cnt2, lc2 = S.subgraph(n, edges, [seeds[q]], 3, rel, cap)
            c = min(cap, int(cnt[q]))
            assert cnt2[0] == c and np.array_equal(ids2[0, :c], ids[q, :c]) and np.array_equal(lv2[0, :c], lv[q, :c])
            assert np.array_equal(lc2[0], lc[q])                                   # never cut


def test_repeats_and_reversed_orientation_give_separate_rows_and_a_self_pair_has_its_vertex_hop():
    edges = K.path_graph(6)
    rel = [[1, 2], [2, 1], [1, 2], [0, 1], [3, 3], [4, 3], [5, 5]]
    ids, lv, cnt, lc = S.subgraph(6, edges, [[0]], 3, rel, 10)
    assert ids[0, :cnt[0]].tolist() == [3, 0, 1, 2, 4] and lv[0, :cnt[0]].tolist() == [1, 2, 2, 2, 3] and lc.tolist() == [[0, 1, 3, 1]]
    ids, lv, cnt, lc = S.subgraph(6, edges, [[3, 3, 4]], 0, rel, 10)                # hops = 0: the relations among the distinct seeds
    assert ids[0, :cnt[0]].tolist() == [4, 5] and lv[0, :2].tolist() == [0, 0] and lc.tolist() == [[2]]


def test_a_row_with_an_end_outside_the_vertices_appears_nowhere():
    n, edges = 5, K.path_graph(5)
    rel = [[0, 1], [-1, 0], [0, 5], [5, 5], [-3, 9], [4, 3]]
    ids, lv, cnt, lc = S.subgraph(n, edges, [[0], [0, 1, 2, 3, 4]], 8, rel, 6)
    assert ids[:, :2].tolist() == [[0, 5], [0, 5]] and cnt.tolist() == [2, 2] and lc.sum(axis=1).tolist() == [2, 2]
    assert np.all(S.row_levels(K.levels(n, edges, [[0, 4]], 8), rel)[0, 1:5] == S.NOT_WITHIN)
