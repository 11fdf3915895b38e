"""EntityGraph.subgraph / neighbourhood_edges / expand_subgraph on the GPU (rarc_khop_edges, csrc/khop.hip) against the
restatement tests/subgraph_ref.py: ids, levels, counts and level counts are equal element for element — the rule is ANDs, ORs and
integer counts, so there is no band.  The shapes are the smallest that reach each path: a relation table of one row, of one
tile exactly and one row to either side, one word of queries and a partial second one, four words, a batch cut at 256, lists
cut at their first entry, inside a level and one short of their size, and rows whose ends name no vertex."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import subgraph_ref as S
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


def _same(got, rl, hops, cap):
    """the edge part of an answer -> the reference row levels"""
    wi, wl, wc = S.listing(rl, cap)
    assert (got.edge_ids.dtype, got.edge_ends.dtype, got.edge_levels.dtype, got.edge_counts.dtype, got.edge_level_counts.dtype) == (
        np.int64, np.int64, np.int32, np.int32, np.int32)
    assert np.array_equal(got.edge_level_counts, S.level_counts(rl, hops)), cap
    assert np.array_equal(got.edge_counts, wc), cap
    assert np.array_equal(got.edge_ids, wi), (cap, np.argwhere(got.edge_ids != wi)[:5])
    assert np.array_equal(got.edge_levels, wl), cap


def _check(g, n, edges, seeds, hops, rows=None, caps=(16384,), lv=None, **kw):
    """neighbourhood_edges at every cap -> the reference; rows=None is the graph's own pair list"""
    lv = K.levels(n, edges, seeds, hops) if lv is None else lv
    table = _own(edges) if rows is None else np.asarray(rows, np.int64)
    rl = S.row_levels(lv, table)
    rel = None if rows is None else _relations(n, table)
    for cap in caps:
        got = g.neighbourhood_edges(seeds, hops=hops, max_edges=cap, relations=rel, **kw)
        _same(got, rl, hops, cap)
        inside = got.edge_ids >= 0
        assert np.array_equal(got.edge_ends[inside], table[got.edge_ids[inside]]) and np.all(got.edge_ends[~inside] == -1)
        assert got.edge_weights is None
    return rl


# ---- small graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [0, 1, 3, 8])
def test_a_path_from_an_end_and_from_the_middle(hops):
    n, edges = 20, K.path_graph(20)
    rl = _check(_graph(n, edges), n, edges, [[0], [10], [19, 0], [10, 11]], hops, caps=(1, 5, 19, 30))
    assert (rl[0] != 255).sum() == hops and (rl[1] != 255).sum() == 2 * hops       # edge (i, i + 1) from vertex 0 has level i + 1
    assert (rl[3] == 0).sum() == 1                                                 # hops = 0: the relation between the two seeds


def test_a_triangle_with_a_tail_the_edge_between_two_hop_1_vertices_is_at_level_1_and_weights_are_gathered():
    n, edges, w = 5, [(0, 1), (0, 2), (2, 1), (2, 3), (3, 4)], [5, 6, 7, 8, 9]
    g = _graph(n, edges, weights=w)
    got = g.neighbourhood_edges([[0]], hops=2, max_edges=8)
    own = _own(edges).tolist()                                                     # (0, 1), (0, 2), (1, 2), (2, 3), (3, 4)
    assert own[2] == [1, 2] and got.edge_ids[0, :got.edge_counts[0]].tolist() == [0, 1, 2, 3]
    assert got.edge_levels[0, :4].tolist() == [1, 1, 1, 2] and got.edge_level_counts.tolist() == [[0, 3, 1]]
    assert got.edge_weights[0].tolist() == [5, 6, 7, 8, 0, 0, 0, 0] and got.edge_ends[0, 2].tolist() == [1, 2]
    _same(got, S.row_levels(K.levels(n, edges, [[0]], 2), own), 2, 8)
    rel = _relations(n, [[2, 1], [4, 3]], weights=np.array([0.5, -2.25], np.float32))
    got = g.neighbourhood_edges([[0], [4]], hops=1, max_edges=2, relations=rel)
    assert got.edge_ids.tolist() == [[0, -1], [1, -1]] and got.edge_levels.tolist() == [[1, -1], [1, -1]]
    assert got.edge_weights.dtype == np.float32 and got.edge_weights.tolist() == [[0.5, 0.0], [-2.25, 0.0]]


def test_the_star_whose_hub_has_259_neighbours_seeded_at_a_leaf():
    n, edges = K.star_graph(259)
    g = _graph(n, edges)
    for hops in (0, 1, 2):
        rl = _check(g, n, edges, [[1], [0], [1, 259]], hops, caps=(1, 258, 259, 300))
        assert (rl[0] != 255).sum() == (0, 1, 259)[hops]


def test_no_seeds_a_repeated_seed_and_unused_slots():
    import torch

    n, edges = 50, K.random_graph(50, 80, 3)[0]
    g = _graph(n, edges)
    rl = _check(g, n, edges, [[], [7, 7, 7], [7], [3, 7, 3]], 2, caps=(1, 80))
    assert np.all(rl[0] == 255) and np.array_equal(rl[1], rl[2])
    slots = torch.tensor([[-1, -1, -1], [-1, 7, -1], [7, 7, 7]], dtype=torch.int64, device="cuda")
    got = g.neighbourhood_edges(slots, hops=2, max_edges=4)
    assert got.edge_counts[0] == 0 and np.all(got.edge_ids[0] == -1) and np.all(got.edge_levels[0] == -1) and np.all(got.edge_level_counts[0] == 0)
    _same(got, S.row_levels(K.levels(n, edges, [[], [7], [7]], 2), _own(edges)), 2, 4)


def _raw(g, seeds, hops, table, max_edges, listed=True):
    """rarc_khop_edges itself, after a traversal -> (ids, levels, count, level_counts) as numpy, or the level counts alone"""
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as KH
    from rag_arc_amd.hip import binding as B

    sd = torch.from_numpy(KH.host_seeds(g.n, seeds)).cuda()
    nq, r = int(sd.shape[0]), len(table)
    ws, wb = KH.traverse(g, sd, hops)
    rel = torch.from_numpy(np.ascontiguousarray(table, np.int64)).cuda()
    ews = torch.empty(int(g.lib.rarc_khop_edges_workspace_bytes(r, nq, hops)), dtype=torch.uint8, device="cuda")
    ids = torch.full((nq, max_edges), 7, dtype=torch.int64, device="cuda")
    lv = torch.full((nq, max_edges), 7, dtype=torch.int32, device="cuda")
    cnt = torch.full((nq,), 7, dtype=torch.int32, device="cuda")
    lc = torch.full((nq, hops + 1), 7, dtype=torch.int32, device="cuda")
    p = (lambda x: x.data_ptr()) if listed else (lambda x: None)
    B.check(g.lib.rarc_khop_edges(g.n, g.m, nq, hops, ws, wb, rel.data_ptr(), r, max_edges, ews.data_ptr(), ews.numel(), p(ids), p(lv), p(cnt),
                                  lc.data_ptr(), None), "rarc_khop_edges")
    torch.cuda.synchronize()
    return (ids.cpu().numpy(), lv.cpu().numpy(), cnt.cpu().numpy(), lc.cpu().numpy()) if listed else lc.cpu().numpy()


def test_repeats_both_orientations_a_self_pair_and_ends_that_name_no_vertex_through_the_binding():
    n, edges = 6, K.path_graph(6)
    table = [[1, 2], [2, 1], [1, 2], [0, 1], [3, 3], [4, 3], [5, 5], [-1, 0], [0, n], [n, n], [-1, -1], [1, 1 << 40], [-(1 << 40), 0], [1, 0]]
    g = _graph(n, edges)
    seeds = [[0], [3, 3, 4], []]
    for hops in (0, 3, 8):
        want = S.subgraph(n, edges, seeds, hops, table, len(table))
        got = _raw(g, seeds, hops, table, len(table))
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), hops
        assert np.array_equal(_raw(g, seeds, hops, table, len(table), listed=False), want[3])    # the count and scan passes alone
        assert not set(got[0].ravel().tolist()) & {7, 8, 9, 10, 11, 12}
    ids, lv, cnt, lc = _raw(g, seeds, 3, table, len(table))
    assert ids[0, :cnt[0]].tolist() == [3, 13, 0, 1, 2, 4] and lv[0, :cnt[0]].tolist() == [1, 1, 2, 2, 2, 3]


# ---- the random graph of the k-hop tests, with a typed relation table of three rows per edge ----------------------------------------------
N, M = 5003, 20011


@pytest.fixture(scope="module")
def world():
    """the graph, 256 seed rows with their reference levels at 3 hops, the table and its row levels: computed once and shared"""
    edges, _ = K.random_graph(N, M, seed=31)
    seeds = K.random_seeds(N, 256, 5, seed=45)
    lv3 = K.levels(N, edges, seeds, 3)
    table = S.typed_relations(edges, seed=32)
    rl3 = S.row_levels(lv3, table)
    for a in (lv3, table, rl3):
        a.setflags(write=False)
    g = _graph(N, edges)
    return {"edges": edges, "g": g, "seeds": seeds, "lv3": lv3, "table": table, "rl3": rl3, "rel": _relations(N, table)}


def _cut(levels, hops):
    """levels at fewer hops (tests/test_gpu_khop.py holds this cut of the dense levels to the reference; max commutes with it)"""
    return np.where(levels <= hops, levels, K.NOT_WITHIN).astype(np.uint8)


def test_the_shared_row_levels_cut_at_fewer_hops_are_the_reference_at_fewer_hops(world):
    for hops in (0, 2):
        lv = K.levels(N, world["edges"], world["seeds"][:9], hops)
        assert np.array_equal(_cut(world["rl3"][:9], hops), S.row_levels(lv, world["table"]))


@pytest.mark.parametrize("nq", [1, 64, 65, 256])
def test_random_graph_with_a_three_times_repeated_table(world, nq):
    assert len(world["table"]) == 3 * M
    for hops in (0, 1, 2, 3):
        got = world["g"].neighbourhood_edges(world["seeds"][:nq], hops=hops, max_edges=300, relations=world["rel"])
        _same(got, _cut(world["rl3"][:nq], hops), hops, 300)
    assert (world["rl3"][:nq] != 255).any()


def test_the_graphs_own_pairs_on_the_random_graph(world):
    rl = S.row_levels(world["lv3"][:70], _own(world["edges"]))
    got = world["g"].neighbourhood_edges(world["seeds"][:70], hops=3, max_edges=500)
    _same(got, rl, 3, 500)
    assert (S.level_counts(world["rl3"][:70], 3) == 3 * S.level_counts(rl, 3)).all()       # the table holds every pair three times


@pytest.mark.parametrize("r", [1, 1023, 1024, 1025])
def test_tables_of_one_row_and_around_one_tile(world, r):
    rows = world["table"][np.argsort(world["rl3"][0], kind="stable")[:r]] if r > 1 else world["table"][np.flatnonzero(world["rl3"][0] == 1)[:1]]
    rl = _check(world["g"], N, world["edges"], world["seeds"][:65], 3, rows=rows, caps=(1, 2000), lv=world["lv3"][:65])
    assert rl.shape == (65, r) and rl[0, -1] != 255                                # the last row of the table is listed


def test_row_q_of_the_256_batch_equals_the_one_query_call_and_a_batch_of_257_is_cut(world):
    g, seeds, rel = world["g"], world["seeds"], world["rel"]
    batch = g.neighbourhood_edges(seeds, hops=3, max_edges=200, relations=rel)
    _same(batch, world["rl3"], 3, 200)
    for q in (0, 1, 63, 64, 65, 255):
        one = g.neighbourhood_edges([seeds[q]], hops=3, max_edges=200, relations=rel)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(one[:5], batch[:5]))
    many = g.neighbourhood_edges(seeds + seeds[:1], hops=2, max_edges=50, relations=rel)
    assert many.edge_ids.shape == (257, 50) and many.edge_ends.shape == (257, 50, 2) and many.edge_level_counts.shape == (257, 3)
    _same(many, _cut(np.concatenate([world["rl3"], world["rl3"][:1]]), 2), 2, 50)


def test_the_cap_cuts_the_list_in_order_and_leaves_the_level_counts(world):
    g, seeds = world["g"], world["seeds"][:3]
    rl = world["rl3"][:3]
    lc = S.level_counts(rl, 3)
    size = int(lc[0].sum())
    assert size > 1200 and lc[0, 2] > 4                                            # (rows of more than one tile are listed)
    caps = (size, size - 1, int(lc[0, :2].sum()) + int(lc[0, 2]) // 2, int(lc[0, :2].sum()), 1)      # exact, one short, inside a level, at its edge
    for cap in caps:
        _same(g.neighbourhood_edges(seeds, hops=3, max_edges=cap, relations=world["rel"]), rl, 3, cap)
    from rag_arc_amd.hip.binding import RarcUnsupported

    with pytest.raises(RarcUnsupported, match="65536"):
        g.neighbourhood_edges(seeds, hops=3, max_edges=65537)
    with pytest.raises(ValueError, match="max_edges"):
        g.neighbourhood_edges(seeds, hops=3, max_edges=0)
    got = g.neighbourhood_edges(seeds, hops=1, max_edges=65536, relations=world["rel"])
    assert got.edge_ids.shape == (3, 65536) and np.array_equal(got.edge_counts, S.level_counts(_cut(rl, 1), 1).sum(axis=1))


def test_a_device_tensor_in_shuffled_order_ids_follow_the_callers_rows(world):
    import torch

    perm = np.random.default_rng(9).permutation(len(world["table"]))
    shuffled = world["table"][perm]
    dev = torch.from_numpy(shuffled).cuda()
    rel = _relations(N, dev)
    assert rel._pairs.data_ptr() == dev.data_ptr()                                 # adopted, not copied
    got = world["g"].neighbourhood_edges(world["seeds"][:70], hops=3, max_edges=400, relations=rel, as_device=True)
    assert got.edge_ids.is_cuda and got.edge_ids.dtype == torch.int64
    host = type(got)(*[x.cpu().numpy() for x in got[:5]])
    _same(host, world["rl3"][:70][:, perm], 3, 400)
    with pytest.raises(ValueError, match="entities"):
        world["g"].neighbourhood_edges([[0]], relations=_relations(N + 1, dev))
    with pytest.raises(ValueError, match="RelationList"):
        world["g"].neighbourhood_edges([[0]], relations=shuffled)


def test_the_vertex_part_of_subgraph_equals_neighbourhood_from_a_separate_call(world):
    g, seeds = world["g"], world["seeds"][:70]
    for early_stop in (False, True):
        sub = g.subgraph(seeds, hops=3, max_vertices=300, max_edges=400, relations=world["rel"], early_stop=early_stop)
        alone = g.neighbourhood(seeds, hops=3, max_vertices=300)
        assert all(np.array_equal(a, b) for a, b in zip(sub[:4], alone))
        _same(sub, world["rl3"][:70], 3, 400)
        edges = g.neighbourhood_edges(seeds, hops=3, max_edges=400, relations=world["rel"])
        assert all(np.array_equal(a, b) for a, b in zip(sub[4:9], edges[:5])) and sub.edge_weights is None
    from rag_arc_amd.encapsulation.database.graph_db import k_hop_subgraph

    one = k_hop_subgraph(N, world["edges"], seeds[:2], hops=2, max_vertices=50, max_edges=60)
    again = g.subgraph(seeds[:2], hops=2, max_vertices=50, max_edges=60)
    assert all(np.array_equal(a, b) for a, b in zip(one[:9], again[:9]))


# ---- seeds from the index ----------------------------------------------------------------------------------------------------------------
def test_expand_subgraph_equals_subgraph_on_the_seeds_the_index_search_returns():
    from rag_arc_amd.hip.engine import FlatIndexF16

    n_ent, dim = 2000, 64
    emb = HashEmbeddings(dim)
    x = np.asarray(emb.embed_documents([f"entity {i}" for i in range(n_ent)]), np.float32)
    edges, _ = K.random_graph(n_ent, 3000, seed=61)
    index = FlatIndexF16(dim, metric="cosine", device=0)
    index.add(x)
    g = _graph(n_ent, edges)
    q = np.asarray([emb.embed_query(t) for t in ("entity 3", "entity 1717", "who founded entity 5")], np.float32)
    _, I = index.search(q, 5)
    seeds = [row.tolist() for row in I]
    rel = _relations(n_ent, S.typed_relations(edges, seed=62, repeats=2))
    for relations in (None, rel):
        a = g.expand_subgraph(index, q, seeds_per_query=5, hops=2, max_vertices=64, max_edges=128, relations=relations)
        b = g.subgraph(seeds, hops=2, max_vertices=64, max_edges=128, relations=relations)
        assert all(np.array_equal(x, y) for x, y in zip(a[:9], b[:9])) and a.edge_counts.min() > 0
    _same(b, S.row_levels(K.levels(n_ent, edges, seeds, 2), rel._pairs.cpu().numpy()), 2, 128)
    with pytest.raises(ValueError):
        g.expand_subgraph(index, q, seeds_per_query=65)
