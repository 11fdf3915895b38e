"""The k-hop subgraph rule of csrc/khop.hip in plain numpy, on top of tests/khop_ref.py: the relations inside a
query's neighbourhood.  Imported by the tests only.

The relation list is r rows (a, b) of int64 in any orientation; a pair may repeat and a may equal b.  With hop_q as
tests/khop_ref.py defines it, row e has level lvl_q(e) = max(hop_q(a), hop_q(b)) and belongs to q's subgraph iff both ends are
within `hops`; a row with an end outside [0, n) belongs to no subgraph.  level_counts[h] = the rows at level h exactly, never
cut.  The list is ordered by (level ascending, row number ascending) and cut at max_edges, (-1, -1) behind.  Edge weights play
no part, and the graph enters only through the dense levels."""
import numpy as np

from tests import khop_ref as K

NOT_WITHIN = K.NOT_WITHIN


def row_levels(lv, relations):
    """uint8 [B][r] from the dense levels uint8 [B][n]: max of the two ends' hops, 255 for a row outside the subgraph"""
    rel = np.asarray(relations, np.int64).reshape(-1, 2)
    n = lv.shape[1]
    ok = (rel >= 0).all(axis=1) & (rel < n).all(axis=1)
    a, b = np.where(ok, rel[:, 0], 0), np.where(ok, rel[:, 1], 0)
    out = np.maximum(lv[:, a], lv[:, b])                                           # 255 is the largest value: one end outside wins
    out[:, ~ok] = NOT_WITHIN
    return out


def level_counts(rl, hops):
    """int32 [B][hops + 1] from the row levels"""
    return K.counts(rl, hops)


def listing(rl, max_edges):
    """(ids int64 [B][max], levels int32 [B][max], count int32 [B]) from the row levels"""
    return K.listing(rl, max_edges)


def subgraph(n, edges, seed_lists, hops, relations, max_edges):
    """-> (ids, levels, count, level_counts) for the graph `edges` and the relation table `relations`"""
    rl = row_levels(K.levels(n, edges, seed_lists, hops), relations)
    return listing(rl, max_edges) + (level_counts(rl, hops),)


def level_bits(lv, relations, hops):
    """The rule as csrc/khop.hip evaluates it, in bits: with S_h(x) = "hop(x) <= h", E_h = S_h(a) & S_h(b) & ~(S_{h-1}(a) &
    S_{h-1}(b)) -> bool [hops + 1][B][r]"""
    rel = np.asarray(relations, np.int64).reshape(-1, 2)
    n = lv.shape[1]
    ok = (rel >= 0).all(axis=1) & (rel < n).all(axis=1)
    a, b = np.where(ok, rel[:, 0], 0), np.where(ok, rel[:, 1], 0)
    out, below = [], np.zeros((lv.shape[0], len(rel)), bool)
    for h in range(hops + 1):
        both = (lv[:, a] <= h) & (lv[:, b] <= h) & ok
        out.append(both & ~below)
        below = both
    return np.stack(out)


def typed_relations(edges, seed, repeats=3):
    """A relation table in the reference's manner: every edge `repeats` times, each copy in a random orientation, the rows
    shuffled -> int64 [repeats * m][2]"""
    rng = np.random.default_rng(seed)
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    rel = np.concatenate([e] * repeats)
    flip = rng.random(len(rel)) < 0.5
    rel[flip] = rel[flip][:, ::-1]
    return rel[rng.permutation(len(rel))]
