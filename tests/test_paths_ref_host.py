"""The connecting-paths reference (tests/paths_ref.py) against networkx.all_shortest_paths: what the GPU tests compare with must
be right before it is a yardstick.  For every pair of vertices with d <= L the on-path vertices and their positions are the
union over networkx's paths, the on-path rows of the graph's own pair list are the union of those paths' edges, and a pair
farther apart than L gives -1 and nothing else."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import paths_ref as P


def _own(edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return np.unique(np.stack([e.min(axis=1), e.max(axis=1)], axis=1), axis=0)


def _against_networkx(n, edges, ends, length):
    """every (a, b) of `ends` as a pair of one-vertex sources -> compared with the union over networkx's shortest paths"""
    nx = pytest.importorskip("networkx")
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(edges)
    vertices = sorted({v for ab in ends for v in ab})
    col = {v: i for i, v in enumerate(vertices)}
    pairs = [(col[a], col[b]) for a, b in ends]
    d, pos = P.paths(n, edges, [[v] for v in vertices], pairs, length)
    own = _own(edges)
    rl = P.row_levels(pos, own)
    row = {tuple(e): i for i, e in enumerate(own.tolist())}
    reachable = 0
    for p, (a, b) in enumerate(ends):
        try:
            found = list(nx.all_shortest_paths(g, a, b))
        except nx.NetworkXNoPath:
            found = []
        if not found or len(found[0]) - 1 > length:
            assert d[p] == -1 and np.all(pos[p] == P.OFF_PATH) and np.all(rl[p] == P.OFF_PATH), (a, b)
            continue
        reachable += 1
        assert d[p] == len(found[0]) - 1
        want = np.full(n, P.OFF_PATH, np.uint8)
        want_rows = np.full(len(own), P.OFF_PATH, np.uint8)
        for path in found:
            for i, v in enumerate(path):
                want[v] = i
            for i, (u, v) in enumerate(zip(path, path[1:])):
                want_rows[row[(min(u, v), max(u, v))]] = i + 1
        assert np.array_equal(pos[p], want), (a, b)
        assert np.array_equal(rl[p], want_rows), (a, b)
    return reachable


@pytest.mark.parametrize("length", [0, 1, 4, 8])
def test_a_path_graph_and_a_cycle(length):
    n = 12
    ends = [(a, b) for a in range(n) for b in range(n)]
    assert _against_networkx(n, K.path_graph(n), ends, length) == sum(1 for a, b in ends if abs(a - b) <= length)
    assert _against_networkx(n, P.cycle_graph(n), ends, length) > 0
    assert _against_networkx(5, P.cycle_graph(5), [(a, b) for a in range(5) for b in range(5)], length) > 0


def test_a_grid_corner_to_corner_holds_every_vertex_at_position_i_plus_j():
    n, edges = 25, P.grid_graph(5, 5)
    d, pos = P.paths(n, edges, [[0], [24]], [(0, 1), (1, 0)], 8)
    assert d.tolist() == [8, 8]
    assert pos[0].tolist() == [i + j for i in range(5) for j in range(5)] and pos[1].tolist() == [8 - i - j for i in range(5) for j in range(5)]
    assert (P.row_levels(pos, _own(edges)) != P.OFF_PATH).all()                    # all 40 edges lie on some shortest path
    assert P.paths(n, edges, [[0], [24]], [(0, 1)], 7)[0].tolist() == [-1]
    ends = [(a, b) for a in range(0, 25, 3) for b in range(25)]
    for length in (2, 8):
        assert _against_networkx(n, edges, ends, length) > 0


@pytest.mark.parametrize("n,m,seed", [(40, 50, 1), (200, 300, 2), (300, 1200, 3)])
def test_random_graphs(n, m, seed):
    edges, _ = K.random_graph(n, m, seed)
    rng = np.random.default_rng(seed)
    ends = [tuple(int(x) for x in rng.integers(0, n, 2)) for _ in range(60)] + [(3, 3)]
    for length in (1, 3, 8):
        assert _against_networkx(n, edges, ends, length) > 0


def test_sets_as_sources_overlap_an_empty_source_a_bad_index_and_the_same_source_twice():
    n, edges = 10, K.path_graph(10)
    sources = [[0, 1], [1, 2], [], [9], [4, 6]]
    pairs = [(0, 1), (0, 2), (2, 2), (0, 3), (3, 0), (3, 3), (0, 5), (-1, 0), (0, 4), (4, 3)]
    d, pos = P.paths(n, edges, sources, pairs, 8)
    assert d.tolist() == [0, -1, -1, 8, 8, 0, -1, -1, 3, 3]
    assert np.flatnonzero(pos[0] != P.OFF_PATH).tolist() == [1]                    # the overlap alone, at position 0
    assert pos[3, 1:].tolist() == list(range(9)) and pos[3, 0] == P.OFF_PATH       # from the nearer end of the set
    assert pos[4].tolist() == [P.OFF_PATH] + [8 - i for i in range(9)]
    assert np.flatnonzero(pos[5] != P.OFF_PATH).tolist() == [9]
    assert pos[8, :5].tolist() == [P.OFF_PATH, 0, 1, 2, 3] and np.all(pos[8, 5:] == P.OFF_PATH)
    assert pos[9, 6:].tolist() == [0, 1, 2, 3]
    assert P.paths(n, edges, sources, [(0, 3)], 7)[0].tolist() == [-1]


def test_rows_repeats_both_orientations_self_pairs_same_position_and_ends_outside_the_vertices():
    # a 4-cycle 0-1-2-3 with a tail 3-4: from 0 to 2 both ways round are shortest, 1 and 3 share position 1
    n, edges = 5, [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4)]
    d, pos = P.paths(n, edges, [[0], [2]], [(0, 1)], 4)
    assert d.tolist() == [2] and pos[0].tolist() == [0, 1, 2, 1, P.OFF_PATH]
    rel = [[0, 1], [1, 0], [0, 1], [1, 3], [1, 1], [0, 2], [2, 3], [3, 4], [-1, 0], [0, 5], [2, 1]]
    rl = P.row_levels(pos, rel)
    assert rl[0].tolist() == [1, 1, 1, 255, 255, 255, 2, 255, 255, 255, 2]          # (0, 2): positions 0 and 2 are not consecutive
    ids, lv, cnt = P.listing(rl, 4)
    assert ids.tolist() == [[0, 1, 2, 6]] and lv.tolist() == [[1, 1, 1, 2]] and cnt.tolist() == [4]
    assert P.counts(rl, 4).tolist() == [[0, 3, 2, 0, 0]] and P.counts(pos, 4).tolist() == [[1, 2, 1, 0, 0]]


def test_a_row_between_consecutive_positions_that_the_graph_lacks_is_on_the_paths_the_table_is_trusted():
    # two routes from 0 to 5, 0-1-2-5 and 0-3-4-5: the cross rows (1, 4) and (2, 3) join position 1 on one route to position 2 on
    # the other and are no edges of the graph
    n, edges = 6, [(0, 1), (1, 2), (2, 5), (0, 3), (3, 4), (4, 5)]
    assert not {(1, 4), (2, 3), (1, 3), (2, 4), (0, 5)} & {tuple(e) for e in _own(edges).tolist()}
    table = [[1, 4], [0, 1], [3, 2], [1, 3], [4, 1], [2, 4], [0, 5], [4, 5]]
    d, pos = P.paths(n, edges, [[0], [5]], [(0, 1), (1, 0)], 3)
    assert d.tolist() == [3, 3] and pos.tolist() == [[0, 1, 2, 1, 2, 3], [3, 2, 1, 2, 1, 0]]
    rl = P.row_levels(pos, table)
    assert rl.tolist() == [[2, 1, 2, 255, 2, 255, 255, 3], [2, 3, 2, 255, 2, 255, 255, 1]]
    ids, lv, cnt = P.listing(rl, 8)
    assert ids[0, :cnt[0]].tolist() == [1, 0, 2, 4, 7] and lv[0, :5].tolist() == [1, 2, 2, 2, 3] and P.counts(rl, 3).tolist() == [[0, 1, 3, 1]] * 2
