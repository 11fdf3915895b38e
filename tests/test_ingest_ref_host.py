"""The ingest rule as tests/ingest_ref.py restates it, against the host constructors' own normalisation
(`_normalise_typed_pairs`, `mention_csr`) on inputs with nothing to skip; the skip kinds and their precedence; unit mode; the
multi-bit base expansion; invariance under row permutation; and what graph_db/ingest.py refuses before it needs a device.  No GPU."""
import numpy as np
import pytest

from tests import ingest_ref as R


def _pagerank():
    from rag_arc_amd.encapsulation.database.graph_db import pagerank

    return pagerank


def _ingest():
    from rag_arc_amd.encapsulation.database.graph_db import ingest

    return ingest


def _random_rows(rng, n, r):
    a = rng.integers(0, n, r)
    b = (a + 1 + rng.integers(0, n - 1, r)) % n                     # never a == b
    return np.stack([a, b], axis=1).astype(np.int64)


def _same_pairs(got, pairs, weights, masks):
    assert np.array_equal(got.pairs, pairs)
    assert (got.weights is None) == (weights is None) and (weights is None or np.array_equal(got.weights.astype(np.int64), weights))
    assert (got.masks is None) == (masks is None) and (masks is None or np.array_equal(got.masks, masks))
    assert got.edges == len(pairs) and not any(got.skipped.values()) and got.base_skipped == 0


# ---- the anchor: the host constructors' normalisation ------------------------------------------------------------------------------
@pytest.mark.parametrize("n, r, seed", [(2, 7, 0), (5, 40, 1), (300, 2500, 2), (70000, 3000, 3)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("typed", [False, True])
def test_pairs_reproduce_the_host_normalisation(n, r, seed, weighted, typed):
    rng = np.random.default_rng(seed)
    rows = _random_rows(rng, n, r)
    w = rng.integers(1, 50, r) if weighted else None
    t = rng.integers(0, 32, r) if typed else None
    _same_pairs(R.ingest_pairs(n, rows, w, t), *_pagerank()._normalise_typed_pairs(n, rows, w, t))


@pytest.mark.parametrize("weighted_base, weighted_rows", [(False, False), (True, True), (True, False), (False, True)])
def test_an_extension_is_the_normalisation_of_the_base_rows_followed_by_the_new_ones(weighted_base, weighted_rows):
    rng = np.random.default_rng(5)
    n = 60
    first = _random_rows(rng, n, 400)
    bp, bw, bm = _pagerank()._normalise_typed_pairs(n, first, rng.integers(1, 9, 400) if weighted_base else None, rng.integers(0, 32, 400))
    order = rng.permutation(len(bp))                                # a base is unique pairs i < j in ANY order
    bp, bm = bp[order], bm[order]
    bw = None if bw is None else bw[order]
    rows, t = _random_rows(rng, n + 10, 300), rng.integers(0, 32, 300)
    w = rng.integers(1, 9, 300) if weighted_rows else None
    got = R.ingest_pairs(n + 10, rows, w, t, base_pairs=bp, base_weights=bw, base_masks=bm)
    # the base as rows: one row per bit of a mask, the weight on the first; the masks through all rows, the weights through the first
    erows, ew, et = R.expand_base(bp, bw, bm)
    assert len(erows) > len(bp)                                     # (some mask has more than one bit)
    all_rows, all_t = np.concatenate([erows, rows]), np.concatenate([et, t])
    pairs, _, masks = _pagerank()._normalise_typed_pairs(n + 10, all_rows, None, all_t)
    if weighted_base or weighted_rows:
        one = lambda k: np.ones(k, np.int64)                        # noqa: E731  (the side without weights counts 1 a row)
        keep = np.ones(len(erows), bool) if ew is None else ew > 0
        first_rows = erows[keep] if bw is not None else bp
        wsum = _pagerank()._normalise_typed_pairs(n + 10, np.concatenate([first_rows, rows]),
                                                  np.concatenate([ew[keep] if bw is not None else one(len(bp)), w if w is not None else one(300)]), None)[1]
    else:
        wsum = None
    _same_pairs(got, pairs, wsum, masks)


def test_a_multi_bit_base_mask_expands_to_one_row_per_bit_with_the_weight_on_the_first():
    rows, w, t = R.expand_base([[0, 1], [2, 5]], [7, 3], [0b1010_0001, 1 << 31])
    assert rows.tolist() == [[0, 1], [0, 1], [0, 1], [2, 5]] and w.tolist() == [7, 0, 0, 3] and t.tolist() == [0, 5, 7, 31]
    got = R.ingest_pairs(6, np.zeros((0, 2), np.int64), None, np.zeros(0, np.int64), base_pairs=[[2, 5], [0, 1]], base_weights=[3, 7],
                         base_masks=[1 << 31, 0b1010_0001])
    assert got.pairs.tolist() == [[0, 1], [2, 5]] and got.weights.tolist() == [7, 3] and got.masks.tolist() == [0b1010_0001, 1 << 31]
    assert (got.largest, got.total) == (7, 10)


@pytest.mark.parametrize("n_chunks, n_entities, r, seed", [(1, 1, 5, 0), (7, 3, 60, 1), (200, 500, 4000, 2)])
@pytest.mark.parametrize("weighted", [False, True])
def test_mentions_reproduce_mention_csr(n_chunks, n_entities, r, seed, weighted):
    from rag_arc_amd.encapsulation.database.graph_db.passages import mention_csr

    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, n_chunks, r), rng.integers(0, n_entities, r)], axis=1)
    w = rng.integers(1, 4, r) if weighted else None
    if n_chunks == 200:
        rows = np.concatenate([rows, np.stack([np.full(70, 3), np.arange(70)], axis=1)])          # a chunk past the split degree
        w = None if w is None else np.concatenate([w, np.ones(70, np.int64)])
    row_ptr, ent, ww, split = mention_csr(n_chunks + 2, n_entities, rows, w)                      # (two trailing empty chunks)
    got = R.ingest_mentions(n_chunks + 2, n_entities, rows, w)
    assert np.array_equal(got.row_ptr, row_ptr) and np.array_equal(got.entities, ent) and got.entities.dtype == np.int32
    assert np.array_equal(got.weights.astype(np.uint32), ww) and np.array_equal(got.split, split)
    assert got.nnz == len(ent) and got.largest == int(ww.max()) and not any(got.skipped.values())
    # an extension: the CSR of the first half as the base, the second half as rows, over more chunks and entities
    half = len(rows) // 2
    base = mention_csr(n_chunks, n_entities, rows[:half], None if w is None else w[:half])[:3]
    ext = R.ingest_mentions(n_chunks + 2, n_entities + 3, rows[half:], None if w is None else w[half:], base=base)
    assert np.array_equal(ext.row_ptr, row_ptr) and np.array_equal(ext.entities, ent) and np.array_equal(ext.weights.astype(np.uint32), ww)
    assert np.array_equal(ext.split, split) and ext.base_skipped == 0


# ---- the skip kinds ------------------------------------------------------------------------------------------------------------------
def test_a_pair_row_is_counted_under_the_first_kind_that_applies():
    rows = [[0, 9], [-1, -1], [3, 3], [9, 9], [1, 2], [1, 2], [2, 1], [4, 0], [0, 4]]
    w = [5, 5, 0, 0, 0, 3, 4, 6, 7]
    t = [0, 40, 40, 40, 40, 32, -1, 31, 0]
    got = R.ingest_pairs(5, rows, w, t)
    #   [0,9] range; [-1,-1] range (not loop); [3,3] loop (not weight, not type); [9,9] range; [1,2] w=0: weight (not type);
    #   [1,2] t=32: type; [2,1] t=-1: type; the last two are the one edge (0, 4)
    assert got.skipped == {"out_of_range": 3, "self_loop": 1, "zero_weight": 1, "bad_type": 2}
    assert got.pairs.tolist() == [[0, 4]] and got.weights.tolist() == [13] and got.masks.tolist() == [(1 << 31) | 1]
    assert (got.edges, got.largest, got.total, got.base_skipped) == (1, 13, 13, 0)
    nothing = R.ingest_pairs(5, [[1, 1], [7, 0]], None, None)
    assert nothing.edges == 0 and nothing.pairs.shape == (0, 2) and (nothing.largest, nothing.total) == (0, 0)


def test_a_base_row_outside_its_contract_is_counted_apart():
    got = R.ingest_pairs(5, [[1, 0]], [2], None, base_pairs=[[0, 1], [2, 1], [3, 3], [0, 5], [2, 4]], base_weights=[4, 1, 1, 1, 0])
    assert got.base_skipped == 4 and not any(got.skipped.values())
    assert got.pairs.tolist() == [[0, 1]] and got.weights.tolist() == [6]


def test_a_mention_row_is_counted_under_the_first_kind_that_applies():
    rows = [[5, 9], [-1, 0], [0, 3], [0, -1], [1, 1], [1, 1], [1, 1], [2, 0]]
    w = [0, 1, 1, 0, 0, 4096, 4095, 1]
    got = R.ingest_mentions(3, 3, rows, w)
    assert got.skipped == {"chunk_out_of_range": 2, "entity_out_of_range": 2, "bad_weight": 2}
    assert got.row_ptr.tolist() == [0, 0, 1, 2] and got.entities.tolist() == [1, 0] and got.weights.tolist() == [4095, 1]
    assert (got.nnz, got.largest) == (2, 4095)
    twice = R.ingest_mentions(3, 3, [[1, 1], [1, 1]], [4095, 1])
    assert twice.largest == 4096 and twice.weights.tolist() == [4096]            # the caller's to refuse
    damaged = R.ingest_mentions(2, 2, [[0, 0]], None, base=([0, 3, 9], [0, 5, 1], [1, 1, 0]))
    assert damaged.base_skipped == 2 and damaged.weights.tolist() == [2] and damaged.row_ptr.tolist() == [0, 1, 1]


# ---- unit mode and permutations ------------------------------------------------------------------------------------------------------
def test_unit_mode_drops_duplicates_and_one_weighted_side_counts_the_other_one_each():
    rows = [[0, 1], [1, 0], [0, 1], [2, 3]]
    unit = R.ingest_pairs(4, rows)
    assert unit.weights is None and unit.pairs.tolist() == [[0, 1], [2, 3]] and (unit.largest, unit.total) == (1, 2)
    ones = R.ingest_pairs(4, rows, [1, 1, 1, 1])
    assert ones.weights.tolist() == [3, 1] and (ones.largest, ones.total) == (3, 4)
    both = R.ingest_pairs(4, rows, None, None, base_pairs=[[0, 1]], base_weights=[10])
    assert both.weights.tolist() == [13, 1]
    other = R.ingest_pairs(4, rows, [2, 2, 2, 2], None, base_pairs=[[2, 3], [0, 1]])
    assert other.weights.tolist() == [7, 3]


def test_the_answer_is_the_same_for_any_order_of_the_rows():
    rng = np.random.default_rng(9)
    rows = np.concatenate([_random_rows(rng, 50, 500), [[3, 3], [70, 1]]])
    w, t = rng.integers(0, 5, 502), rng.integers(-1, 33, 502)
    a = R.ingest_pairs(50, rows, w, t)
    p = rng.permutation(502)
    b = R.ingest_pairs(50, rows[p], w[p], t[p])
    assert a.skipped == b.skipped and all(a.skipped.values())
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    mrows = np.stack([rng.integers(-1, 9, 300), rng.integers(-1, 6, 300)], axis=1)
    mw = rng.integers(0, 6, 300)
    q = rng.permutation(300)
    c, d = R.ingest_mentions(8, 5, mrows, mw), R.ingest_mentions(8, 5, mrows[q], mw[q])
    assert c.skipped == d.skipped and all(c.skipped.values())
    for x, y in zip(c[:4], d[:4]):
        assert x.tobytes() == y.tobytes()


# ---- what Python refuses before it needs a device -----------------------------------------------------------------------------------
def _fake_graph(n, m, typed):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    g = EntityGraph.__new__(EntityGraph)
    g.n, g.m, g.device = n, m, "cuda:0"
    g._type_masks = object() if typed else None
    return g


def _fake_map(n_chunks, n_entities, nnz):
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    x = MentionMap.__new__(MentionMap)
    x.n_chunks, x.n_entities, x.nnz, x.device = n_chunks, n_entities, nnz, "cuda:0"
    return x


def test_mixed_typed_and_untyped_extensions_are_refused():
    with pytest.raises(ValueError, match="the graph carries relation types and the rows do not"):
        _fake_graph(5, 3, True).extended([[0, 1]])
    with pytest.raises(ValueError, match="the rows carry relation types and the graph does not"):
        _fake_graph(5, 3, False).extended([[0, 1]], types=[2])


def test_an_extension_never_shrinks():
    with pytest.raises(ValueError, match="smaller than the graph's 5 vertices"):
        _fake_graph(5, 3, False).extended([[0, 1]], n=4)
    with pytest.raises(ValueError, match="smaller than the map's 4 chunks"):
        _fake_map(4, 6, 9).extended([[0, 1]], n_chunks=3)
    with pytest.raises(ValueError, match="smaller than the map's 6 entities"):
        _fake_map(4, 6, 9).extended([[0, 1]], n_entities=5)


def test_shapes_dtypes_and_limits_are_refused():
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph, MentionMap
    from rag_arc_amd.hip import binding as B

    for rows in ([0, 1], [[0, 1, 2]], [[0.5, 1.0]], np.zeros((2, 2, 2), np.int64)):
        with pytest.raises(ValueError, match="rows|mentions"):
            EntityGraph.from_rows(5, rows)
        with pytest.raises(ValueError, match="rows|mentions"):
            MentionMap.from_rows(5, 5, rows)
    for kw in ({"weights": [1]}, {"weights": [1, -1]}, {"weights": [1, 1 << 32]}, {"weights": [0.5, 1]}, {"types": [1]}, {"types": [0.5, 1]},
               {"types": [True, False]}, {"on_invalid": "ignore"}):
        with pytest.raises(ValueError):
            EntityGraph.from_rows(5, [[0, 1], [1, 2]], **kw)
    for kw in ({"weights": [1]}, {"weights": [1, -1]}, {"on_invalid": None}):
        with pytest.raises(ValueError):
            MentionMap.from_rows(5, 5, [[0, 1], [1, 2]], **kw)
    for n in (1, 0, -3):
        with pytest.raises(ValueError, match="at least 2 vertices"):
            EntityGraph.from_rows(n, [[0, 1]])
    with pytest.raises(B.RarcUnsupported, match="2\\^31 - 1"):
        EntityGraph.from_rows((1 << 31) - 1, [[0, 1]])
    with pytest.raises(ValueError, match="at least 1 chunk"):
        MentionMap.from_rows(0, 5, [[0, 1]])
    with pytest.raises(ValueError, match="at least 1 entity"):
        MentionMap.from_rows(5, 0, [[0, 1]])
    with pytest.raises(B.RarcUnsupported, match="n_chunks"):
        MentionMap.from_rows((1 << 31) - 1, 5, [[0, 1]])
    # base + new rows reach 2^31: refused from the counts alone
    with pytest.raises(B.RarcUnsupported, match="base \\+ new rows < 2\\^31"):
        _fake_graph(5, (1 << 31) - 2, False).extended([[0, 1], [1, 2]])
    with pytest.raises(B.RarcUnsupported, match="base \\+ new rows < 2\\^31"):
        _fake_map(4, 6, (1 << 31) - 1).extended([[0, 1]])
    I = _ingest()
    assert I.check_values([3, -1, 1 << 40], 3, "types", signed=True).tolist() == [3, -1, -1]      # a type the kernel will count as bad
    assert I.check_values([0, (1 << 32) - 1], 2, "weights", signed=False).view(np.uint32).tolist() == [0, (1 << 32) - 1]
    assert (I.PAIR_KINDS, I.MENTION_KINDS) == (R.PAIR_KINDS, R.MENTION_KINDS)


def test_a_relation_list_refuses_rows_of_another_kind():
    from rag_arc_amd.encapsulation.database.graph_db import RelationList

    def fake(weights, typed):
        x = RelationList.__new__(RelationList)
        x.n_entities, x.r, x.device = 5, 3, "cuda:0"
        x._weights, x._types = (object() if weights else None), (object() if typed else None)
        return x

    with pytest.raises(ValueError, match="the rows carry weights and the relation list does not"):
        fake(False, False).extended([[0, 1]], weights=[1.5])
    with pytest.raises(ValueError, match="the relation list carries weights and the rows do not"):
        fake(True, False).extended([[0, 1]])
    with pytest.raises(ValueError, match="the rows carry types and the relation list does not"):
        fake(False, False).extended([[0, 1]], types=[1])
    with pytest.raises(ValueError, match="the relation list carries types and the rows do not"):
        fake(False, True).extended([[0, 1]])
    with pytest.raises(ValueError, match="smaller than the list's 5 entities"):
        fake(False, False).extended([[0, 1]], n_entities=4)
    with pytest.raises(ValueError, match="relation type"):
        fake(False, True).extended([[0, 1]], types=[32])


def test_no_cpu_fallback():
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph, MentionMap
    from rag_arc_amd.hip import binding as B

    if torch.cuda.is_available():
        assert EntityGraph.from_rows(3, [[1, 0], [0, 1]]).m == 1 and MentionMap.from_rows(2, 2, [[1, 0], [1, 0]]).nnz == 1
        return
    for call in (lambda: EntityGraph.from_rows(3, [[1, 0]]), lambda: MentionMap.from_rows(2, 2, [[1, 0]])):
        with pytest.raises(B.RarcError, match="no CPU fallback"):
            call()


def test_the_limits_are_the_python_constants():
    I = _ingest()
    assert I.limits() == {"types": 32, "mention_weight_bits": 12, "split_degree": 64, "max_count": I.MAX_COUNT}
