"""EntityGraph.shortest_paths / path_chunks / connect on the GPU (rarc_khop_paths and rarc_khop_path_edges, csrc/khop.hip) against the
restatement tests/paths_ref.py: distances, positions, lists, counts, row levels and chunk scores are equal element for element —
the rule is ANDs, ORs, integer minima and counts, so there is no band.  The shapes are the smallest that reach each path: one
word of sources or pairs, one column more and four words, columns of a pair in different words, lists cut at their first entry,
inside a level and one short of their size, a relation table of one row, one tile and one row to either side."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import passage_ref as M
from tests import paths_ref as P
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu


def _graph(n, edges, **kw):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, edges, **kw)


def _relations(n, rows, **kw):
    from rag_arc_amd.encapsulation.database.graph_db import RelationList

    return RelationList(n, rows, **kw)


def _own(edges):
    """the graph's own relation list: the pairs as EntityGraph normalises them (i < j, sorted, each once)"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return np.unique(np.stack([e.min(axis=1), e.max(axis=1)], axis=1), axis=0)


def _same(got, d, pos, rl, length, vcap, ecap):
    """an answer -> the reference distances, dense positions and row levels"""
    assert [x.dtype for x in got[:10]] == [np.int32, np.int64, np.int32, np.int32, np.int32, np.int64, np.int64, np.int32, np.int32, np.int32]
    assert np.array_equal(got.distances, d), (got.distances, d)
    wi, wp, wc = P.listing(pos, vcap)
    assert np.array_equal(got.position_counts, P.counts(pos, length)), vcap
    assert np.array_equal(got.vertex_counts, wc) and np.array_equal(got.vertex_ids, wi) and np.array_equal(got.vertex_positions, wp), vcap
    wi, wl, wc = P.listing(rl, ecap)
    assert np.array_equal(got.edge_level_counts, P.counts(rl, length)), ecap
    assert np.array_equal(got.edge_counts, wc), ecap
    assert np.array_equal(got.edge_ids, wi), (ecap, np.argwhere(got.edge_ids != wi)[:5])
    assert np.array_equal(got.edge_levels, wl), ecap


def _check(g, n, edges, sources, pairs, length, rows=None, caps=((64, 64),), lv=None, **kw):
    """shortest_paths at every (max_vertices, max_edges) -> the reference; rows=None is the graph's own pair list"""
    lv = K.levels(n, edges, sources, length) if lv is None else lv
    d, pos = P.positions(lv, pairs, length)
    table = _own(edges) if rows is None else np.asarray(rows, np.int64)
    rl = P.row_levels(pos, table)
    rel = None if rows is None else _relations(n, table)
    for vcap, ecap in caps:
        got = g.shortest_paths(sources, pairs, max_length=length, max_vertices=vcap, max_edges=ecap, relations=rel, **kw)
        _same(got, d, pos, rl, length, vcap, ecap)
        inside = got.edge_ids >= 0
        assert np.array_equal(got.edge_ends[inside], table[got.edge_ids[inside]]) and np.all(got.edge_ends[~inside] == -1)
    return d, pos, rl


# ---- small graphs ---------------------------------------------------------------------------------------------------------------------
def test_two_vertices_and_one_edge():
    g = _graph(2, [(0, 1)])
    for length in (0, 1, 8):
        d, pos, rl = _check(g, 2, [(0, 1)], [[0], [1], [0, 1]], [(0, 1), (1, 0), (0, 0), (2, 0), (2, 2)], length, caps=((1, 1), (2, 2), (5, 5)))
        assert d.tolist() == [1 if length else -1, 1 if length else -1, 0, 0, 0]
    assert pos.tolist() == [[0, 1], [1, 0], [0, 255], [0, 255], [0, 0]] and rl.tolist() == [[1], [1], [255], [255], [255]]


@pytest.mark.parametrize("length", [0, 3, 4, 8])
def test_a_path_graph_at_the_bound_and_one_past_it(length):
    n, edges = 20, K.path_graph(20)
    sources = [[0], [length], [length + 1], [10], [19, 0], [10, 11], []]
    pairs = [(0, 1), (0, 2), (1, 0), (3, 3), (3, 5), (4, 3), (5, 4), (0, 6), (6, 6), (4, 4)]
    d, pos, rl = _check(_graph(n, edges), n, edges, sources, pairs, length, caps=((1, 1), (5, 5), (20, 19), (30, 30)), early_stop=True)
    assert d[:4].tolist() == [length, -1, length, 0] and d[4] == 0 and d[7:].tolist() == [-1, -1, 0]      # d == L is kept, L + 1 is not
    assert np.flatnonzero(pos[0] != 255).tolist() == list(range(length + 1)) and (rl[0] != 255).sum() == length
    assert np.flatnonzero(pos[4] != 255).tolist() == [10]                          # overlapping sets: the common vertex alone
    assert d[5] == -1 and d[6] == (8 if length == 8 else -1)                       # 9 from {19, 0} to 10; 8 from 11 to 19, the nearer ends


def test_two_components_a_cycle_with_a_longer_way_round_and_a_grid():
    n, edges = K.two_components_and_isolated()
    d, pos, _ = _check(_graph(n, edges), n, edges, [[0], [3], [6], [9], [12], [2]], [(0, 1), (0, 2), (2, 3), (4, 0), (4, 4), (0, 5)], 4)
    assert d.tolist() == [3, -1, 2, -1, 0, 2]
    assert (pos[0] != 255).sum() == 6 and pos[5].tolist()[:6] == [0, 1, 2, 255, 255, 255]      # 0 -> 3 both ways round; 0 -> 2 one way
    n, edges = 5, P.cycle_graph(5)
    d, pos, rl = _check(_graph(n, edges), n, edges, [[0], [2]], [(0, 1)], 8)
    assert d.tolist() == [2] and pos.tolist() == [[0, 1, 2, 255, 255]] and (rl != 255).sum() == 2
    n, edges = 25, P.grid_graph(5, 5)
    d, pos, rl = _check(_graph(n, edges), n, edges, [[0], [24]], [(0, 1), (1, 0)], 8, caps=((1, 1), (24, 39), (25, 40)))
    assert d.tolist() == [8, 8] and pos[0].tolist() == [i + j for i in range(5) for j in range(5)] and (rl != 255).all()
    assert _check(_graph(n, edges), n, edges, [[0], [24]], [(0, 1)], 7)[0].tolist() == [-1]


@pytest.mark.parametrize("leaves", [65, 300])
def test_a_star_from_leaf_to_leaf(leaves):
    n, edges = K.star_graph(leaves)
    d, pos, rl = _check(_graph(n, edges), n, edges, [[1], [leaves], [0], [1, 2, 3]], [(0, 1), (0, 2), (1, 1), (3, 1)], 2, caps=((1, 1), (3, 2), (8, 8)))
    assert d.tolist() == [2, 1, 0, 2] and np.flatnonzero(pos[0] != 255).tolist() == [0, 1, leaves] and (rl[0] != 255).sum() == 2
    assert (pos[3] != 255).sum() == 5                                              # three leaves, the hub, the far leaf


# ---- the random graph: batch shapes ----------------------------------------------------------------------------------------------------
N, M_EDGES = 3000, 6000


@pytest.fixture(scope="module")
def world():
    """the graph, 256 sources with their reference levels at 8 hops, computed once and shared"""
    edges, _ = K.random_graph(N, M_EDGES, seed=71)
    rng = np.random.default_rng(72)
    sources = [[int(v) for v in rng.integers(0, N, size=1 + q % 3)] for q in range(256)]
    sources[7] = []
    sources[9] = sources[8][:1] + sources[9]                                       # overlaps source 8
    lv8 = K.levels(N, edges, sources, 8)
    lv8.setflags(write=False)
    return {"edges": edges, "g": _graph(N, edges), "sources": sources, "lv8": lv8, "own": _own(edges)}


def _cut(levels, hops):
    """levels at fewer hops (tests/test_gpu_khop.py holds this cut of the dense levels to the reference)"""
    return np.where(levels <= hops, levels, K.NOT_WITHIN).astype(np.uint8)


def _pairs(ns, npairs, seed):
    """npairs pairs over ns sources: the two ends of the column range, a column with itself, a repeated pair, then random ones"""
    rng = np.random.default_rng(seed)
    fixed = [(0, ns - 1), (ns - 1, 0), (ns // 2, ns // 2), (0, ns - 1), (min(8, ns - 1), min(9, ns - 1))]
    rest = [tuple(int(x) for x in rng.integers(0, ns, 2)) for _ in range(npairs)]
    return (fixed + rest)[:npairs]


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("npairs", [1, 64, 65, 256])
def test_batches_of_every_word_count_of_sources_and_pairs(world, ns, npairs):
    pairs = _pairs(ns, npairs, seed=ns * 1000 + npairs)
    if ns == 256 and npairs >= 64:
        assert any(a >> 6 != b >> 6 for a, b in pairs) and pairs[0] == pairs[3]    # columns in different words; a repeated pair
    d, pos, _ = _check(world["g"], N, world["edges"], world["sources"][:ns], pairs, 4, caps=((50, 60),), lv=_cut(world["lv8"][:ns], 4))
    assert npairs < 64 or ns == 1 or ((d > 0).any() and (d == -1).any())


def test_row_p_of_the_256_batch_equals_the_one_pair_call(world):
    g, sources = world["g"], world["sources"]
    pairs = _pairs(256, 256, seed=5)
    batch = g.shortest_paths(sources, pairs, max_length=5, max_vertices=40, max_edges=40)
    d, pos = P.positions(_cut(world["lv8"], 5), pairs, 5)
    _same(batch, d, pos, P.row_levels(pos, world["own"]), 5, 40, 40)
    for p in (0, 3, 4, 63, 64, 65, 255):
        one = g.shortest_paths(sources, [pairs[p]], max_length=5, max_vertices=40, max_edges=40)
        assert all(np.array_equal(a[0], b[p]) for a, b in zip(one[:10], batch[:10])), p
        ia, ib = pairs[p]
        two = g.shortest_paths([sources[ia], sources[ib]], [(0, 1)], max_length=5, max_vertices=40, max_edges=40)
        assert all(np.array_equal(a[0], b[p]) for a, b in zip(two[:10], batch[:10])), p


@pytest.mark.parametrize("length", [4, 8])
def test_the_caps_cut_the_lists_in_order_and_leave_the_counts(world, length):
    lv = _cut(world["lv8"], length)
    d, pos = P.positions(lv[:40], [(a, b) for a in range(0, 40, 2) for b in (a + 1,)], length)
    p = int(np.argmax((pos != 255).sum(axis=1)))                                   # the pair with the most vertices on its paths
    pair = [(2 * p, 2 * p + 1)]
    d, pos = P.positions(lv, pair, length)
    rl = P.row_levels(pos, world["own"])
    pc, lc = P.counts(pos, length)[0], P.counts(rl, length)[0]
    vsize, esize = int(pc.sum()), int(lc.sum())
    assert d[0] >= 2 and vsize >= d[0] + 1 and esize >= d[0]
    caps = ((1, 1), (int(pc[0]) + 1, int(lc[1]) + 1), (vsize - 1, esize - 1), (vsize, esize), (vsize + 3, esize + 3))
    _check(world["g"], N, world["edges"], world["sources"], pair, length, caps=caps, lv=lv)
    from rag_arc_amd.hip.binding import RarcUnsupported

    for kw in ({"max_vertices": 65537}, {"max_edges": 65537}, {"max_length": 9}):
        with pytest.raises(RarcUnsupported):
            world["g"].shortest_paths(world["sources"], pair, **kw)
    for kw in ({"max_vertices": 0}, {"max_edges": 0}, {"max_length": -1}):
        with pytest.raises(ValueError):
            world["g"].shortest_paths(world["sources"], pair, **kw)
    with pytest.raises(ValueError, match="outside"):
        world["g"].shortest_paths(world["sources"], [(0, 256)])
    with pytest.raises(ValueError, match="outside"):
        world["g"].shortest_paths([[N]], [(0, 0)])


@pytest.mark.parametrize("n", [1023, 1024, 1025])
def test_vertex_counts_around_one_tile(n):
    edges, _ = K.random_graph(n, 2 * n, seed=n)
    sources = [[q * 13 % n] for q in range(69)] + [[n - 1]]
    pairs = [(q, 69 - q) for q in range(70)] + [(69, 69)]
    d, pos, _ = _check(_graph(n, edges), n, edges, sources, pairs, 4, caps=((30, 40),))
    assert (d > 0).any() and (pos[:, n - 1] != 255).any()                          # the last vertex is on some path


def test_the_same_bits_under_a_permutation_of_the_edges_and_from_device_tensors(world):
    import torch

    edges = np.asarray(world["edges"], np.int64)
    shuffled = edges[np.random.default_rng(3).permutation(len(edges))][:, ::-1]
    pairs = _pairs(256, 100, seed=6)
    a = world["g"].shortest_paths(world["sources"], pairs, max_length=4, max_vertices=30, max_edges=30)
    b = _graph(N, shuffled.tolist()).shortest_paths(world["sources"], pairs, max_length=4, max_vertices=30, max_edges=30)
    assert all(np.array_equal(x, y) for x, y in zip(a[:10], b[:10]))
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as KH

    sd = torch.from_numpy(KH.host_seeds(N, world["sources"])).cuda()
    for dtype in (torch.int32, torch.int64):
        c = world["g"].shortest_paths(sd, torch.tensor(pairs, dtype=dtype, device="cuda"), max_length=4, max_vertices=30, max_edges=30, as_device=True)
        assert c.vertex_ids.is_cuda and all(np.array_equal(x, y.cpu().numpy()) for x, y in zip(a[:10], c[:10])) and c.edge_weights is None
    with pytest.raises(ValueError, match="outside"):
        world["g"].shortest_paths(sd, torch.tensor([[0, 256]], device="cuda"))


# ---- relation tables -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 1023, 1024, 1025])
def test_tables_of_one_row_and_around_one_tile(world, r):
    lv = _cut(world["lv8"], 6)
    pairs = _pairs(256, 65, seed=8)
    d, pos = P.positions(lv, pairs, 6)
    p = int(np.argmax(d))
    full = P.row_levels(pos, world["own"])
    order = np.argsort(full[p], kind="stable")                                     # the rows on pair p's paths first
    rows = world["own"][order[:r]][:, ::-1] if r > 1 else world["own"][order[:1]]
    rows = np.roll(rows, -1, axis=0)                                               # an on-path row is the last of the table
    _, _, rl = _check(world["g"], N, world["edges"], world["sources"], pairs, 6, rows=rows, caps=((20, 1), (20, 2000)), lv=lv)
    assert rl.shape == (65, r) and rl[p, 0] != 255 and rl[p, -1] != 255


def _raw(g, sources, pairs, length, table, max_edges, listed=True):
    """rarc_khop_paths, then rarc_khop_levels / rarc_khop_counts / rarc_khop_path_edges on the state it wrote -> numpy"""
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as KH
    from rag_arc_amd.hip import binding as B

    sd = torch.from_numpy(KH.host_seeds(g.n, sources)).cuda()
    pd = torch.tensor(pairs, dtype=torch.int32, device="cuda")                     # (unchecked: indices outside [0, ns) reach the kernels)
    npairs, r = len(pairs), len(table)
    dist, pws, pwb = KH.mark_paths(g, sd, pd, length)
    dense = torch.full((npairs, g.n), 7, dtype=torch.uint8, device="cuda")
    B.check(g.lib.rarc_khop_levels(g.n, g.m, npairs, length, pws, pwb, dense.data_ptr(), None), "rarc_khop_levels")
    pc = torch.full((npairs, length + 1), 7, dtype=torch.int32, device="cuda")
    B.check(g.lib.rarc_khop_counts(g.n, g.m, npairs, length, pws, pwb, pc.data_ptr(), None), "rarc_khop_counts")
    rel = torch.from_numpy(np.ascontiguousarray(table, np.int64)).cuda()
    ews = torch.empty(int(g.lib.rarc_khop_edges_workspace_bytes(r, npairs, length)), dtype=torch.uint8, device="cuda")
    ids = torch.full((npairs, max_edges), 7, dtype=torch.int64, device="cuda")
    lv = torch.full((npairs, max_edges), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((npairs,), 7, dtype=torch.int32, device="cuda")
    lc = torch.full((npairs, length + 1), 7, dtype=torch.int32, device="cuda")
    p = (lambda x: x.data_ptr()) if listed else (lambda x: None)
    B.check(g.lib.rarc_khop_path_edges(g.n, g.m, npairs, length, pws, pwb, rel.data_ptr(), r, max_edges, ews.data_ptr(), ews.numel(), p(ids), p(lv),
                                       p(cnt), lc.data_ptr(), None), "rarc_khop_path_edges")
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (dist, dense, pc, ids, lv, cnt, lc))


def test_repeats_orientations_self_pairs_same_position_rows_skipped_positions_and_bad_pair_indices_through_the_binding():
    # a 4-cycle 0-1-2-3 with a tail 3-4-5: from 0 to 2 both ways round are shortest, 1 and 3 share position 1
    n, edges = 6, [(0, 1), (1, 2), (2, 3), (0, 3), (3, 4), (4, 5)]
    table = [[0, 1], [1, 0], [0, 1], [1, 3], [1, 1], [0, 2], [2, 3], [3, 4], [-1, 0], [0, n], [n, n], [1, 1 << 40], [-(1 << 40), 0], [2, 1],
             [5, 3], [3, 5], [0, 0]]                                               # (1, 3) joins one position; (3, 5) is no edge of the graph
    g = _graph(n, edges)
    sources = [[0], [2], [5], [], [0, 5]]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 2), (0, 3), (0, 5), (-1, 0), (5, 5), (4, 1), (1 << 20, 0)]
    for length in (0, 2, 3, 8):
        d, pos = P.paths(n, edges, sources, pairs, length)
        rl = P.row_levels(pos, table)
        wi, wl, wc = P.listing(rl, len(table))
        dist, dense, pc, ids, lv, cnt, lc = _raw(g, sources, pairs, length, table, len(table))
        assert np.array_equal(dist, d) and np.array_equal(dense, pos) and np.array_equal(pc, P.counts(pos, length)), length
        assert np.array_equal(ids, wi) and np.array_equal(lv, wl) and np.array_equal(cnt, wc) and np.array_equal(lc, P.counts(rl, length)), length
        assert np.array_equal(_raw(g, sources, pairs, length, table, len(table), listed=False)[6], lc)      # the count and scan passes alone
        assert not set(ids.ravel().tolist()) & {3, 4, 5, 8, 9, 10, 11, 12, 16} and np.all(lc[:, 0] == 0)
    assert dist.tolist() == [2, 2, 3, 0, -1, -1, -1, -1, 2, -1]
    assert ids[0, :cnt[0]].tolist() == [0, 1, 2, 6, 13] and lv[0, :cnt[0]].tolist() == [1, 1, 1, 2, 2]
    assert ids[2, :cnt[2]].tolist() == [7] and lv[2, :cnt[2]].tolist() == [2]      # 0-3-4-5: (0, 3) is not in the table, (3, 5) skips a position
    d2 = _raw(g, sources, pairs, 2, table, 4)
    assert d2[0].tolist() == [2, 2, -1, 0, -1, -1, -1, -1, 2, -1] and d2[5][2] == 0 and np.all(d2[1][2] == 255)


def test_a_row_between_consecutive_positions_that_the_graph_lacks_is_listed_the_table_is_trusted():
    # two routes from 0 to 5, 0-1-2-5 and 0-3-4-5: positions 0 | 1, 3 | 2, 4 | 5.  The cross rows (1, 4) and (2, 3) join position 1 on
    # one route to position 2 on the other and are no edges of the graph; (1, 3) and (2, 4) join one position, (0, 5) positions 0 and 3
    n, edges = 6, [(0, 1), (1, 2), (2, 5), (0, 3), (3, 4), (4, 5)]
    assert not {(1, 4), (2, 3), (1, 3), (2, 4), (0, 5)} & {tuple(e) for e in _own(edges).tolist()}
    table = [[1, 4], [0, 1], [3, 2], [1, 3], [4, 1], [2, 4], [0, 5], [4, 5]]
    g = _graph(n, edges)
    d, pos, rl = _check(g, n, edges, [[0], [5]], [(0, 1), (1, 0)], 3, rows=table, caps=((6, 1), (6, 4), (6, 8)))
    assert d.tolist() == [3, 3] and pos[0].tolist() == [0, 1, 2, 1, 2, 3]
    assert rl.tolist() == [[2, 1, 2, 255, 2, 255, 255, 3], [2, 3, 2, 255, 2, 255, 255, 1]]
    got = g.shortest_paths([[0], [5]], [(0, 1)], max_length=3, max_vertices=6, max_edges=8, relations=_relations(n, table))
    assert got.edge_ids[0, :got.edge_counts[0]].tolist() == [1, 0, 2, 4, 7] and got.edge_levels[0, :5].tolist() == [1, 2, 2, 2, 3]
    assert got.edge_ends[0, 1].tolist() == [1, 4] and got.edge_level_counts.tolist() == [[0, 1, 3, 1]]
    dist, dense, pc, ids, lv, cnt, lc = _raw(g, [[0], [5]], [(0, 1)], 3, table, 8)                 # and through the binding, the CSR unread
    assert dist.tolist() == [3] and ids[0, :cnt[0]].tolist() == [1, 0, 2, 4, 7] and lv[0, :5].tolist() == [1, 2, 2, 2, 3] and lc.tolist() == [[0, 1, 3, 1]]


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("length,decay", [(4, None), (0, None), (3, [100, 0, 65536, 1])])
def test_path_chunks_and_their_top_k(length, decay):
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    n, n_chunks = 400, 301
    edges, _ = K.random_graph(n, 700, seed=51)
    mentions, weights = M.random_mentions(n, n_chunks - 1, seed=52, max_degree=9, max_weight=30)
    big, big_w = M.chunk_of_degree(n, 150, seed=53, chunk=n_chunks - 1, max_weight=20)      # one chunk of more than 64 mentions
    mentions, weights = mentions + big, weights + big_w
    g, mm = _graph(n, edges), MentionMap(n_chunks, n, mentions, weights=weights)
    sources = K.random_seeds(n, 69, 2, seed=54) + [[]]
    pairs = _pairs(70, 66, seed=55)
    d, pos = P.paths(n, edges, sources, pairs, length)
    table = K.default_decay(length) if decay is None else decay
    want = P.chunk_scores(pos, n_chunks, mentions, weights, table)
    got = g.path_chunks(mm, sources, pairs, max_length=length, decay=decay)
    assert got.dtype == np.float64 and got.shape == (66, n_chunks) and np.array_equal(_bits(got), _bits(want)) and (want > 0).any()
    for k in (1, 10):
        ids, sc, cnt = g.path_chunks(mm, sources, pairs, max_length=length, decay=decay, top_k=k)
        for p in range(len(pairs)):
            wi, wsc, wc = K.chunk_topk([int(x) for x in np.rint(want[p] * K.SCORE_ONE)], k)
            assert cnt[p] == wc and ids[p].tolist() == wi and _bits(sc[p]).tolist() == _bits(wsc).tolist(), (k, p)
    with pytest.raises(ValueError, match="decay"):
        g.path_chunks(mm, sources, pairs, max_length=length, decay=[1] * (length + 2))


# ---- seeds from the index ----------------------------------------------------------------------------------------------------------------
def test_connect_equals_shortest_paths_on_the_seeds_the_index_search_returns():
    from rag_arc_amd.hip.engine import FlatIndexF16

    n_ent, dim = 2000, 64
    emb = HashEmbeddings(dim)
    x = np.asarray(emb.embed_documents([f"entity {i}" for i in range(n_ent)]), np.float32)
    edges, _ = K.random_graph(n_ent, 5000, seed=61)
    index = FlatIndexF16(dim, metric="cosine", device=0)
    index.add(x)
    g = _graph(n_ent, edges, weights=[1 + i % 5 for i in range(len(edges))])
    q = np.asarray([emb.embed_query(f"entity {i * 37}") for i in range(30)], np.float32)
    _, I = index.search(q, 5)
    sources = [[int(v)] for row in I for v in row]
    pairs = [(qi * 5 + i, qi * 5 + j) for qi in range(30) for i in range(5) for j in range(i + 1, 5)]
    got = g.connect(index, q, seeds_per_query=5, max_length=4, max_vertices=32, max_edges=48)            # 30 queries: two launches of 25 and 5
    assert got.distances.shape == (300,) and got.pair_query.tolist() == [p // 10 for p in range(300)] and got.pair_query.dtype == np.int32
    assert np.array_equal(got.pair_ends, np.asarray([[sources[a][0], sources[b][0]] for a, b in pairs], np.int64))
    for q0 in (0, 25):
        part = [(a - q0 * 5, b - q0 * 5) for a, b in pairs[q0 * 10:(q0 + 25) * 10]]
        want = g.shortest_paths(sources[q0 * 5:(q0 + 25) * 5], part, max_length=4, max_vertices=32, max_edges=48)
        assert all(np.array_equal(a[q0 * 10:(q0 + 25) * 10], b) for a, b in zip(got[:11], want[:11])) and want.edge_weights is not None
    d, pos = P.paths(n_ent, edges, sources, pairs, 4)
    _same(got, d, pos, P.row_levels(pos, _own(edges)), 4, 32, 48)
    assert (d > 0).any() and got.edge_weights.shape == (300, 48) and got.edge_weights[got.edge_ids < 0].sum() == 0
    two = g.connect(index, q[:1], seeds_per_query=2, relations=_relations(n_ent, _own(edges)[::-1].copy()))
    assert two.distances.shape == (1,) and two.edge_weights is None and two.pair_ends.tolist() == [I[0, :2].tolist()]
    with pytest.raises(ValueError):
        g.connect(index, q, seeds_per_query=1)
