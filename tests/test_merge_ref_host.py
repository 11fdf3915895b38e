"""tests/merge_ref.py, the numpy restatement of the entity-merging rule, held to a dict-and-loop restatement on
random small inputs and to hand-worked cases.  No GPU, no library."""
import numpy as np
import pytest

from tests import merge_ref as R


# ---- the rule once more, with dicts and loops ---------------------------------------------------------------------------------------
def loop_plan(labels, rich):
    n = len(labels)
    members = {}
    for v in range(n):
        members.setdefault(int(labels[v]), []).append(v)
    primary = [0] * n
    for vs in members.values():
        best = vs[0]
        for v in vs:                                       # ascending: a tie keeps the smaller index
            if rich[v] > rich[best]:
                best = v
        for v in vs:
            primary[v] = best
    kept = [v for v in range(n) if primary[v] == v]
    number = {v: i for i, v in enumerate(kept)}
    return primary, [number[primary[v]] for v in range(n)], kept, [v for v in range(n) if primary[v] != v]


def loop_pairs(new_id, pairs, w):
    acc, dropped, dropped_w = {}, 0, 0
    for (a, b), x in zip(pairs, w):
        a, b = new_id[a], new_id[b]
        if a == b:
            dropped, dropped_w = dropped + 1, dropped_w + int(x)
            continue
        key = (min(a, b), max(a, b))
        acc[key] = acc.get(key, 0) + int(x)
    keys = sorted(acc)
    return [list(k) for k in keys], [acc[k] for k in keys], dropped, dropped_w


def loop_mentions(new_id, ment, w):
    acc = {}
    for (c, e), x in zip(ment, w):
        acc[(int(c), new_id[e])] = acc.get((int(c), new_id[e]), 0) + int(x)
    keys = sorted(acc)
    return [list(k) for k in keys], [acc[k] for k in keys]


def loop_relations(new_id, rel):
    n, table, rows, internal, out = len(new_id), [], [], 0, 0
    for i, (a, b) in enumerate(rel):
        if not (0 <= a < n and 0 <= b < n):
            out += 1
        elif a != b and new_id[a] == new_id[b]:
            internal += 1
        else:
            table.append([new_id[a], new_id[b]])
            rows.append(i)
    return table, rows, internal, out


@pytest.mark.parametrize("seed", range(12))
def test_the_reference_equals_the_loops_on_random_small_inputs(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    labels = rng.integers(0, n, n) if seed % 3 else R.planted_labels(n, n // 4, seed)
    rich = rng.integers(0, 3, n) if seed % 2 else rng.integers(0, 1 << 32, n)
    got = R.plan(labels, rich)
    primary, new_id, kept, removed = loop_plan(labels, rich)
    assert (got["primary"].tolist(), got["new_id"].tolist(), got["kept"].tolist(), got["removed"].tolist()) == (primary, new_id, kept, removed)
    assert got["n_merged"] == len(kept) == len(set(labels.tolist())) and got["n"] == n
    assert np.array_equal(R.plan(labels)["primary"], np.asarray(loop_plan(labels, [0] * n)[0]))
    pairs = rng.integers(0, n, (60, 2))
    w = rng.integers(1, 1 << 20, 60)
    gp, gw, gd, gdw = R.merge_pairs(new_id, pairs, w)
    assert (gp.tolist(), gw.tolist(), gd, gdw) == loop_pairs(new_id, pairs.tolist(), w)
    ment = np.stack([rng.integers(0, 9, 80), rng.integers(0, n, 80)], axis=1)
    mw = rng.integers(1, 30, 80)
    gm, gmw, gmax = R.merge_mentions(new_id, 9, ment, mw)
    assert (gm.tolist(), gmw.tolist()) == loop_mentions(new_id, ment.tolist(), mw) and gmax == max(gmw)
    rel = rng.integers(-1, n + 1, (70, 2))
    gt, gr, gi, go = R.merge_relations(new_id, rel)
    assert (gt.tolist(), gr.tolist(), gi, go) == loop_relations(new_id, rel.tolist())
    keys = rng.integers(0, 20, 100).astype(np.uint64)
    vals = rng.integers(0, 1 << 32, 100).astype(np.uint64)
    uk, us, umax = R.sort_reduce(keys, vals)
    assert uk.tolist() == sorted(set(keys.tolist())) and us.tolist() == [int(vals[keys == k].sum()) for k in uk] and umax == max(us.tolist())


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------------
def test_a_richness_tie_goes_to_the_smallest_index_and_a_primary_need_not_be_its_label():
    p = R.plan([3, 3, 3, 3, 4], [1, 5, 5, 0, 0])            # class {0, 1, 2, 3} labelled 3: 1 and 2 tie at 5
    assert p["primary"].tolist() == [1, 1, 1, 1, 4] and p["kept"].tolist() == [1, 4] and p["removed"].tolist() == [0, 2, 3]
    assert p["new_id"].tolist() == [0, 0, 0, 0, 1] and p["n_merged"] == 2
    p = R.plan([2, 2, 2])                                   # no richness: the smallest member, not the label
    assert p["primary"].tolist() == [0, 0, 0] and p["kept"].tolist() == [0]


def test_an_internal_pair_is_dropped_and_two_pairs_collapse_into_one_with_added_weights():
    new_id = R.plan([0, 0, 2, 3])["new_id"]                 # {0, 1} -> 0, 2 -> 1, 3 -> 2
    pairs, w, dropped, dropped_w = R.merge_pairs(new_id, [(0, 1), (0, 2), (1, 2), (2, 3)], [10, 3, 4, 5])
    assert pairs.tolist() == [[0, 1], [1, 2]] and w.tolist() == [7, 5] and (dropped, dropped_w) == (1, 10)
    pairs, w, dropped, _ = R.merge_pairs(new_id, [(0, 1)])
    assert pairs.shape == (0, 2) and w.size == 0 and dropped == 1


def test_a_relation_a_equals_b_on_a_removed_entity_stays_on_the_merged_one():
    new_id = R.plan([0, 0, 2], [9, 1, 0])["new_id"]         # 1 is removed onto 0
    table, rows, internal, out = R.merge_relations(new_id, [(1, 1), (1, 0), (2, 1), (1, 3), (0, 0)])
    assert table.tolist() == [[0, 0], [1, 0], [0, 0]] and rows.tolist() == [0, 2, 4] and (internal, out) == (1, 1)


def test_a_mention_sum_reaching_2_to_the_12_minus_1_and_2_to_the_12():
    new_id = [0, 0, 1]
    m, w, largest = R.merge_mentions(new_id, 2, [(1, 0), (1, 1), (0, 2)], [4000, 95, 1])
    assert m.tolist() == [[0, 1], [1, 0]] and w.tolist() == [1, 4095] and largest == R.MAX_MENTION_WEIGHT - 1
    assert R.merge_mentions(new_id, 2, [(1, 0), (1, 1), (0, 2)], [4000, 96, 1])[2] == R.MAX_MENTION_WEIGHT


def test_the_identity_labelling_returns_every_input_unchanged():
    rng = np.random.default_rng(2)
    n = 30
    p = R.plan(np.arange(n), rng.integers(0, 9, n))
    assert all(p[k].tolist() == list(range(n)) for k in ("primary", "new_id", "kept")) and p["removed"].size == 0 and p["n_merged"] == n
    e = rng.integers(0, n, (200, 2))
    pairs = np.unique(np.sort(e[e[:, 0] != e[:, 1]], axis=1), axis=0)
    w = rng.integers(1, 100, len(pairs))
    gp, gw, dropped, dropped_w = R.merge_pairs(p["new_id"], pairs, w)
    assert np.array_equal(gp, pairs) and np.array_equal(gw, w) and (dropped, dropped_w) == (0, 0)
    ment = np.unique(np.stack([rng.integers(0, 7, 100), rng.integers(0, n, 100)], axis=1), axis=0)
    mw = rng.integers(1, 100, len(ment))
    gm, gmw, _ = R.merge_mentions(p["new_id"], 7, ment, mw)
    assert np.array_equal(gm, ment) and np.array_equal(gmw, mw)
    table, rows, internal, out = R.merge_relations(p["new_id"], e)
    assert np.array_equal(table, e) and rows.tolist() == list(range(len(e))) and (internal, out) == (0, 0)
