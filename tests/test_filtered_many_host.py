"""The host side of search_filtered_many (hip/engine.py; no GPU): grouping by RowSet identity, the tile table of
rarc_search_rows_grouped — no tile spans a group, the tiles cover every query once, the offsets are the concatenation's — and
the leg rule on hand cases."""
import types

import numpy as np
import pytest

from rag_arc_amd.hip.engine import (FlatIndexF16, build_tile_table, filtered_many_plan, group_rowsets, grouped_tile_queries)

SIZES = [0, 1, 31, 33, 5000, 32768, 32769, 70_001]
COUNTS = [1, 7, 8, 9]


def test_grouping_is_by_identity_in_order_of_first_appearance():
    a, b, c = object(), object(), [1]
    same_as_c = [1]                                      # equal, not identical: a group of its own
    groups = group_rowsets([a, b, a, None, b, c, None, same_as_c, a])
    assert [g for g, _ in groups] == [a, b, None, c, same_as_c]
    assert [p for _, p in groups] == [[0, 2, 8], [1, 4], [3, 6], [5], [7]]
    assert group_rowsets([]) == []
    assert sorted(i for _, p in groups for i in p) == list(range(9))


def test_queries_per_tile():
    assert grouped_tile_queries(1, 128) == 1 and grouped_tile_queries(1, 4096) == 1
    assert grouped_tile_queries(2, 128) == 8 and grouped_tile_queries(256, 2048) == 8
    assert grouped_tile_queries(2, 2176) == 4 and grouped_tile_queries(256, 4096) == 4


@pytest.mark.parametrize("qt", [1, 4, 8])
def test_tile_table_on_the_size_lists(qt):
    counts = [c for _ in SIZES for c in COUNTS]
    ms = [m for m in SIZES for _ in COUNTS]
    if qt == 1:
        counts, ms = [1], [32769]
    tiles, offs = build_tile_table(counts, ms, qt)
    assert tiles.dtype == np.int64 and tiles.shape[1] == 4 and offs.dtype == np.int64
    # the offsets are those of the lists laid one behind the other
    assert offs.tolist() == np.concatenate([[0], np.cumsum(ms)[:-1]]).tolist()
    first = np.concatenate([[0], np.cumsum(counts)])     # group g holds queries [first[g], first[g + 1])
    covered = np.zeros(sum(counts), dtype=int)
    for q0, n, off, m in tiles.tolist():
        assert 1 <= n <= qt
        g = int(np.searchsorted(first, q0, side="right")) - 1
        assert first[g] <= q0 and q0 + n <= first[g + 1], "a tile spans two groups"
        assert off == offs[g] and m == ms[g]
        covered[q0: q0 + n] += 1
    assert (covered == 1).all()
    assert len(tiles) == sum(-(-c // qt) for c in counts)
    assert tiles[:, 0].tolist() == sorted(tiles[:, 0].tolist())


def test_tile_table_hand_cases():
    tiles, offs = build_tile_table([9, 1, 8], [33, 0, 5], 8)
    assert tiles.tolist() == [[0, 8, 0, 33], [8, 1, 0, 33], [9, 1, 33, 0], [10, 8, 33, 5]] and offs.tolist() == [0, 33, 33]
    tiles, _ = build_tile_table([5, 3], [700, 1500], 4)
    assert tiles.tolist() == [[0, 4, 0, 700], [4, 1, 0, 700], [5, 3, 700, 1500]]
    tiles, offs = build_tile_table([], [], 8)
    assert tiles.shape == (0, 4) and offs.size == 0
    with pytest.raises(ValueError):
        build_tile_table([0], [5], 8)


def _index_like(ntotal):
    fake = types.SimpleNamespace(ntotal=ntotal, FILTER_OVERFETCH_MAX_K=FlatIndexF16.FILTER_OVERFETCH_MAX_K,
                                 FILTER_SUBSET_WORK=FlatIndexF16.FILTER_SUBSET_WORK)
    fake._overfetch_k = lambda k, m: FlatIndexF16._overfetch_k(fake, k, m)
    fake.filter_strategy = lambda nq, k, m: FlatIndexF16.filter_strategy(fake, nq, k, m)
    fake._filter_kprime = lambda k, m: FlatIndexF16._filter_kprime(fake, k, m)
    return fake


def test_the_leg_rule_on_hand_cases():
    n = 1_000_000
    idx = _index_like(n)
    plan = lambda sizes, k, strategy: filtered_many_plan(sizes, k, strategy, idx.filter_strategy, idx._filter_kprime)      # noqa: E731
    # "auto" is filter_strategy per group, unchanged: 1 % of the rows for one query -> the list (1e4 * 33 <= 8e6); half of
    # them -> over-fetch at k' = ceil(1.5 * 10 * 2) + 32 = 62; a thousandth would need k' = 15032 > 8192 -> the list
    legs, kp = plan([(1, 10_000), (1, 500_000), (1, 1_000), (3, None)], 10, "auto")
    assert legs == ["subset", "overfetch", "subset", "overfetch"] and kp == 62
    assert [idx.filter_strategy(1, 10, m) for m in (10_000, 500_000, 1_000)] == legs[:3]
    # the group's OWN query count decides: 256 queries over 3 % of the rows are past the threshold, one query is not
    assert plan([(256, 30_000)], 10, "auto")[0] == ["overfetch"] and plan([(1, 30_000)], 10, "auto")[0] == ["subset"]
    # the largest k' of the leg serves all of it; unfiltered queries alone ask for k
    assert plan([(2, 500_000), (2, 250_000), (1, None)], 10, "auto") == (["overfetch", "overfetch", "overfetch"], 92)
    assert plan([(4, None)], 7, "auto") == (["overfetch"], 7)
    assert plan([(4, 1_000)], 7, "auto") == (["subset"], 0)
    # an empty filter is the list's (padding), whatever the rest does
    assert plan([(1, 0), (1, 500_000)], 10, "auto")[0] == ["subset", "overfetch"]
    # forced strategies apply to every filtered group; unfiltered queries always take the ordinary search; k' is clamped
    assert plan([(1, 10_000), (1, 500_000), (1, None)], 10, "subset") == (["subset", "subset", "overfetch"], 10)
    legs, kp = plan([(1, 10_000), (1, 0), (1, None)], 10, "overfetch")
    assert legs == ["overfetch"] * 3 and kp == 8192
    small = _index_like(50)
    assert filtered_many_plan([(1, 1)], 10, "overfetch", small.filter_strategy, small._filter_kprime) == (["overfetch"], 50)
    assert filtered_many_plan([(1, 1)], 100, "overfetch", small.filter_strategy, small._filter_kprime) == (["overfetch"], 100)
