"""The planted BM25 cases of tests/bm25_plant.py, proven from the reference alone (no GPU): every case run by
tests/test_gpu_bm25_select.py is what its name says: its merge rounds, where its winners lie, which exit of the final select
its cut takes, that its tie spans the named seam, that its last tile is short, that its token order matters."""
import itertools

import numpy as np
import pytest

from tests import bm25_plant as P
from tests.bm25_plant import T


def test_rounds_tiles_and_groups():
    assert P.rounds(8 * T, 1024) == [8]
    assert P.rounds(8 * T + 1, 1024) == [9, 2]
    assert P.rounds(64 * T, 1024) == [64, 8]
    assert P.rounds(65 * T - 5, 1024) == [65, 9, 2]
    assert P.rounds(65 * T - 5, 1000) == [65, 9, 2] and 8 * 1000 < T          # 8000 real items and padding
    assert P.rounds(65 * T - 5, 683) == [65, 6] and T // 683 == 11 and 11 * 683 < T
    assert P.rounds(65 * T - 5, 3) == [65] and T // 3 == 2730
    assert P.rounds(65 * T - 5, 1) == [65] and P.rounds(1, 1) == [1]
    assert P.rounds(65 * T, 129) == [65, 2] and T // 129 == 63
    assert P.rounds(1_000_000, 100) == [123, 2]                              # the existing suite's deepest plan
    assert P.tile_of(T - 1) == 0 and P.tile_of(T) == 1
    assert P.group_of(8 * T - 1, 1024) == 0 and P.group_of(8 * T, 1024) == 1
    assert P.group_of(64 * T - 1, 1024, 1) == 0 and P.group_of(64 * T, 1024, 1) == 1
    assert max(c.n_docs for c in map(P.case, P.BUILDERS)) <= 65 * T


@pytest.mark.parametrize("name", list(P.BUILDERS))
def test_planted_values_are_inside_the_contract(name):
    c = P.case(name)
    assert max(c.ks) <= min(P.MAX_K, c.n_docs)
    for q, terms in enumerate(c.queries):
        s = c.scores(q)
        assert np.isfinite(s).all() and not (np.signbit(s) & (s == 0)).any(), (name, q)
        if len(terms) == 1 and c.idf[terms[0]] == 1.0:       # the reference of a one-token query is the planted vector
            assert np.array_equal(P.bits(s), P.bits(c.vectors[terms[0]])), (name, q)
        if not terms:
            assert not s.any() and np.array_equal(c.order(q, max(c.ks)), np.arange(max(c.ks)))
    for v in c.vectors:
        assert np.isfinite(v).all() and not (np.signbit(v) & (v == 0)).any(), name
    idx = c.index()
    assert idx.n_docs == c.n_docs and idx.n_terms == len(c.vectors)
    for t in range(idx.n_terms):
        d = idx.post_doc[idx.post_off[t]:idx.post_off[t + 1]]
        assert np.all(np.diff(d) > 0) and (d.size == 0 or (d[0] >= 0 and d[-1] < c.n_docs))
        assert np.array_equal(P.bits(idx.post_w[idx.post_off[t]:idx.post_off[t + 1]]), P.bits(c.vectors[t][d]))


@pytest.mark.parametrize("shape", list(P.MERGE_SHAPES))
def test_merge_depth_cases(shape):
    n = P.MERGE_SHAPES[shape]
    c = P.case(f"merge_{shape}")
    nt = P.tiles(n)
    n_last = n - (nt - 1) * T
    want_rounds = {"8T": [8], "8T+1": [9, 2], "64T": [64, 8], "65T-5": [65, 9, 2]}[shape]
    assert P.rounds(n, 1024) == want_rounds
    if shape == "8T":
        assert nt * 1024 == T                                  # one final merge, every item slot real
    if shape == "8T+1":
        assert n_last == 1                                     # the lone list of the first round is a one-document tile
    if shape == "64T":
        assert nt == 8 * (T // 1024)                           # 8 full groups, then 8 * 1024 real items in the final merge
    if shape == "65T-5":
        assert n_last == T - 5
    for k in P.MERGE_KS:
        # winners of term 0: the k best are distinct, lie at the end of the corpus, the best of all is the last document
        s, o = c.scores(P.Q_LAST), c.order(P.Q_LAST, k)
        assert P.cut(s, k) == (1, 0) and o[0] == n - 1 and o.min() >= n - 1024
        if n_last >= 1024:
            assert np.all(P.tile_of(o) == nt - 1)              # all k in the last tile
        if nt % 8 == 1:                                        # ... which is the lone last list of the first round
            assert np.all(P.group_of(o[:min(k, n_last)], 1024) == want_rounds[1] - 1) and (nt - 1) % 8 == 0
        if shape == "65T-5":                                   # and of the second round's input at k = 1024
            assert np.all(P.group_of(o, 1024, 0) == 8) and want_rounds[1] % 8 == 1
        assert not np.array_equal(o, np.sort(o)) or k == 1     # the answer's order is not the id order
        # winners of term 1: round-robin over the tiles
        s, o = c.scores(P.Q_ROBIN), c.order(P.Q_ROBIN, k)
        if shape != "8T+1":
            assert P.cut(s, k) == (1, 0)
            per_tile = np.bincount(P.tile_of(o), minlength=nt)
            assert per_tile.max() - per_tile.min() <= 1 and np.array_equal(P.tile_of(o[:min(k, nt)]), np.arange(min(k, nt)))
        else:                                                   # the one-document tile holds one winner, the rest 0.0
            assert (s > 0).sum() == 1024 - (1024 // nt - 1) and s[8 * T] > 0
            assert P.tile_of(o[:min(k, nt)]).tolist() == list(range(min(k, nt)))
        # a mix of signs in every tile
        for v in c.vectors:
            for t in range(nt):
                assert (v[t * T:(t + 1) * T] < 0).any() or n_last == 1 and t == nt - 1
        # the empty query: everything 0.0, the tie runs through every tile and group
        s = c.scores(P.Q_EMPTY)
        assert P.cut(s, k) == (k, n - k)


@pytest.mark.parametrize("sign", ["pos", "neg"])
def test_tie_cases(sign):
    c = P.case(f"ties_{sign}")
    v = 2.5 if sign == "pos" else -2.5
    s = c.scores(P.Q_TIED)
    assert (s == v).sum() == 130 and np.array_equal(np.flatnonzero(s == v), P.TIE_DOCS)
    assert (s > v).sum() == 3 and np.all(P.tile_of(np.flatnonzero(s > v)) == 64)
    if sign == "neg":                                           # the untouched documents (0.0) rank above the tie
        assert not s[s > v].any() and (s < v).sum() == c.n_docs - 133
    else:
        assert (s == 0).sum() == c.n_docs - 133
    seams = {}
    for name, k in P.TIE_KS.items():
        assert P.cut(s, k) == (k - 3, 130 - (k - 3)) and k < 130          # tied, more tied documents than k
        o = c.order(P.Q_TIED, c.n_docs)
        last_in, first_out = int(o[k - 1]), int(o[k])
        assert s[last_in] == v == s[first_out] and last_in < first_out
        assert np.array_equal(np.sort(o[3:k]), P.TIE_DOCS[:k - 3])        # the lowest ids of the tie
        seams[name] = (last_in, first_out, k)
        # the variant with distinct values: the k-th value is unique, the same documents win
        u = c.scores(P.Q_UNIQUE)
        assert P.cut(u, k) == (1, 0) and np.array_equal(np.sort(c.order(P.Q_UNIQUE, k)), np.sort(o[:k]))
    a, b, k = seams["inside_tile"]
    assert P.tile_of(a) == P.tile_of(b) and (a % T, b % T) == (0, T - 1)
    a, b, k = seams["tile_edge"]
    assert b == a + 1 and P.tile_of(b) == P.tile_of(a) + 1 and P.group_of(a, k) == P.group_of(b, k)
    a, b, k = seams["group_edge"]
    assert b == a + 1 and P.rounds(c.n_docs, k) == [65, 2] and (P.group_of(a, k), P.group_of(b, k)) == (0, 1)
    # inside every tile the select of the tile kernel is tied too: two (five) documents above a run of equal scores
    for t in range(65):
        tile = s[t * T:(t + 1) * T]
        if sign == "pos":
            assert (tile == 0).sum() == T - (5 if t == 64 else 2)


def test_all_equal_cases():
    for name, n in (("equal_T", T), ("equal_8T", 8 * T)):
        c = P.case(name)
        assert c.n_docs == n and n % T == 0                    # no placeholder slot in any tile
        for q, v in ((0, 2.5), (1, -2.5), (2, 0.0)):
            assert np.all(c.scores(q) == v)
            for k in c.ks:
                assert P.cut(c.scores(q), k) == (k, n - k)
                assert np.array_equal(c.order(q, k), np.arange(k))
    assert P.rounds(8 * T, 1024) == [8] and P.case("equal_8T").ks == (1024,)      # a full final merge of equal keys


@pytest.mark.parametrize("k", P.SHORT_KS)
def test_short_last_tile_cases(k):
    assert P.short_r(k) == (1, 5, k - 1, k, k + 1)
    for r in P.short_r(k):
        c = P.case(f"short_T+{r}_k{k}")
        assert c.n_docs == T + r and P.tiles(c.n_docs) == 2 and c.ks == (k,)
        assert (r < k) == (r in (1, 5, k - 1))                 # placeholders enter the last tile's list iff r < k
        top = c.order(P.Q_TOP, k)
        assert (top >= T).sum() == min(r, k)                   # the answer is the last tile's documents first
        assert np.all(top[:min(r, k)] >= T)
        bottom = c.order(P.Q_BOTTOM, k)
        assert (bottom >= T).sum() == 0 and (c.scores(P.Q_BOTTOM)[T:] < c.scores(P.Q_BOTTOM)[:T].min()).all()
        assert P.cut(c.scores(P.Q_TOP), k) == (1, 0) == P.cut(c.scores(P.Q_BOTTOM), k)
        below = c.scores(P.Q_TOP_BELOW_ZERO)                   # every score negative, the same winners in the same order
        assert (below < 0).all() and np.array_equal(c.order(P.Q_TOP_BELOW_ZERO, k), top)
    for name, n in (("small_1024", 1024), ("small_1", 1), ("small_T", T), ("small_T+1", T + 1)):
        c = P.case(name)
        assert c.n_docs == n and max(c.ks) == min(n, 1024)
        s = c.scores(0)
        assert np.unique(s).size == n and (n == 1 or ((s < 0).any() and (s > 0).any()))


@pytest.mark.parametrize("name", ["keys_T", "keys_3T"])
def test_key_order_cases(name):
    c = P.case(name)
    s = c.scores(0)
    assert P.tiles(c.n_docs) == (1 if name == "keys_T" else 3)
    sp, run = P.special_values(), P.consecutive_run()
    assert sp.size == 12 and set(sp.tolist()) == {x * g for g in (1, -1) for x in (
        P.DBL_MAX, P.MIN_SUB, P.MIN_NORMAL, 1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53)}
    assert P.MIN_SUB == float(np.array([1], dtype=np.uint64).view(np.float64)[0]) and P.MIN_NORMAL == 2.0 ** -1022
    assert run.size == P.RUN and np.all(np.diff(run.view(np.int64)) == 1) and run.min() < -1e-300 < run.max()
    assert np.all(np.diff(np.sort(run).view(np.int64)) == -1)               # one ulp apart, no gap
    for x in np.concatenate([sp, run]):
        assert (P.bits(s) == P.bits([x])[0]).sum() == 1
    assert (s == 0).sum() == P.KEY_UNTOUCHED
    o = c.order(0, c.n_docs)
    assert s[o[:6]].tolist() == [P.DBL_MAX, 1.0 + 2.0 ** -52, 1.0, 1.0 - 2.0 ** -53, P.MIN_NORMAL, P.MIN_SUB]
    assert not s[o[6:11]].any() and s[o[11:13]].tolist() == [-P.MIN_SUB, -P.MIN_NORMAL]
    assert np.array_equal(s[o[13:13 + P.RUN]], np.sort(run)[::-1])           # then the run, then everything else
    assert s[o[-4:]].tolist() == [-(1.0 - 2.0 ** -53), -1.0, -(1.0 + 2.0 ** -52), -P.DBL_MAX]
    assert P.KEY_ABOVE_RUN == 13
    for k in (P.KEY_KS[2], 1024):                                            # the cut lies inside the run
        assert 13 < k < 13 + P.RUN and P.cut(s, k) == (1, 0)
        assert P.bits(s[o[k - 1]]) - P.bits(s[o[k]]) in (1, -1 % 2 ** 64)
    if name == "keys_3T":                                                   # specials and run reach all three tiles
        where = P.tile_of(o[:13 + P.RUN])
        assert set(where.tolist()) == {0, 1, 2}
    for t in range(P.tiles(c.n_docs)):
        tile = s[t * T:(t + 1) * T]
        assert (tile > 0).any() and (tile < 0).any()


def test_summation_order_case():
    c = P.case("sum_order")
    qs = {tuple(q): i for i, q in enumerate(c.queries)}
    for t0 in (0, 3, 6):
        perms = list(itertools.permutations(range(t0, t0 + 3)))
        base = c.scores(qs[perms[0]])
        differ = [p for p in perms[1:] if not np.array_equal(P.bits(c.scores(qs[p])), P.bits(base))]
        assert differ, t0                                        # another token order gives other bits
    a, b, na = c.vectors[0], c.vectors[1], c.vectors[2]
    full = np.flatnonzero((a != 0) & (b != 0) & (na != 0))
    # (a + b) - a != (a - a) + b wherever b is no multiple of a's ulp: everywhere but a = 1e16 (ulp 2) with b = 2
    differ = c.scores(qs[(0, 1, 2)])[full] != c.scores(qs[(0, 2, 1)])[full]
    assert np.array_equal(differ, ~((a[full] == 1e16) & (b[full] == 2.0))) and differ.mean() > 0.9
    assert np.all(c.scores(qs[(0, 2, 1)])[full] == b[full])
    for t in range(3):                                           # negative idf on positive weights: the same products
        at = c.vectors[t] != 0
        assert np.array_equal(at, c.vectors[t + 3] != 0)
        assert np.array_equal(P.bits(c.idf[t] * c.vectors[t][at]), P.bits(c.idf[t + 3] * c.vectors[t + 3][at]))
    for p in itertools.permutations(range(3)):
        assert np.array_equal(P.bits(c.scores(qs[p])), P.bits(c.scores(qs[tuple(t + 3 for t in p)])))
    assert c.idf[5] == -1.0 and (c.vectors[5] >= 0).all() and (c.vectors[5] > 0).any()
    subsets = {tuple(bool(v[d] != 0) for v in c.vectors[:3]) for d in range(c.n_docs)}
    assert len(subsets) >= 6 and (True, True, True) in subsets and (False, True, False) in subsets
    assert [0, 0, 1] in c.queries and any(len(set(q)) < len(q) for q in c.queries)
    # the products of terms 6-8 round: a fused multiply-add would give other bits somewhere
    s = c.scores(qs[(6, 7, 8)])
    exact = [float(c.idf[t]) * c.vectors[t].astype(np.longdouble) for t in (6, 7, 8)]
    fused = ((np.float64(exact[0]).astype(np.longdouble) + exact[1]).astype(np.float64).astype(np.longdouble)
             + exact[2]).astype(np.float64)
    if np.finfo(np.longdouble).nmant > 52:
        assert (fused != s).any()
    assert P.tiles(c.n_docs) == 3 and c.ks == (P.SUM_K,)


def test_long_run_case():
    c = P.case("long_runs")
    idx = c.index()
    per_tile = [np.bincount(P.tile_of(idx.post_doc[idx.post_off[t]:idx.post_off[t + 1]]), minlength=3).tolist()
                for t in range(2)]
    assert per_tile == [[T, T, T - 9], [0, 2049, 0]]
    assert T == 4 * 4 * 512 and 2049 == 4 * 512 + 1              # four full trips of 4 x 512 postings; one trip and one over
    assert c.queries[0] == [0, 1] and c.queries[1] == [1, 0]
    assert (c.idf < 0).any() and (c.idf > 0).any()
