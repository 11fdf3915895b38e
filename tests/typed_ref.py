"""The typed-traversal rule of csrc/khop.hip in plain Python / numpy, on top of tests/khop_ref.py,
tests/subgraph_ref.py and tests/paths_ref.py: k-hop over the relation types a query allows.  Imported by the tests only.

A type is an integer t in [0, 32).  The mask M(u, v) of an undirected pair {u, v} is the OR of 1 << t over the relations that
join u and v, in either orientation.  Query q carries a filter F_q (a uint32) and may cross {u, v} iff M(u, v) & F_q != 0 — an
edge of mask 0 is crossed by nobody.  hop_q(v) is the fewest crossable edges from any seed of q to v; a seed has hop 0 whatever
its filter, and v is in q's neighbourhood iff hop_q(v) <= hops.  That is a breadth-first search of each query over its own
filtered edge set, which is what `levels` runs.

A relation row (a, b, t) is in q's subgraph at level max(hop_q(a), hop_q(b)) iff that level is <= hops, F_q holds t and both ends
lie in [0, n); a row whose t lies outside [0, 32) is in no subgraph.  (A row that carries a mask, as the graph's own pairs do,
needs mask & F_q != 0.)  Paths: one filter F for the whole call; every source traverses under F, and a path-edge row additionally
needs F to hold its type."""
import numpy as np

from tests import khop_ref as K
from tests import paths_ref as P
from tests import subgraph_ref as S

NOT_WITHIN = K.NOT_WITHIN
ALL = 0xFFFFFFFF
N_TYPES = 32


def filter_mask(types):
    """an iterable of type ids -> the filter with their bits"""
    f = 0
    for t in types:
        assert 0 <= int(t) < N_TYPES
        f |= 1 << int(t)
    return f


def edge_masks(pairs, types):
    """input pairs [k][2] in any orientation, repeats allowed, and one type per pair -> (pairs int64 [m][2] with i < j, each
    once, ascending; masks uint32 [m]): the OR of 1 << t over the inputs that join a pair"""
    acc = {}
    for (a, b), t in zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(), types):
        key = (min(a, b), max(a, b))
        acc[key] = acc.get(key, 0) | (1 << int(t))
    keys = sorted(acc)
    return np.array(keys, np.int64).reshape(-1, 2), np.array([acc[k] for k in keys], np.uint32)


def levels_one(n, pairs, masks, seeds, f, hops):
    """uint8 [n]: one query's breadth-first search over the edges its filter crosses"""
    kept = [tuple(e) for e, mk in zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(), masks) if int(mk) & int(f)]
    return K.levels_one(n, kept, seeds, hops)


def levels(n, pairs, masks, seed_lists, filters, hops):
    """uint8 [B][n]: levels_one for every query (tests/test_typed_ref_host.py holds the two equal); the queries of one filter
    share a filtered edge set and one frontier matrix"""
    pairs, masks = np.asarray(pairs, np.int64).reshape(-1, 2), np.asarray(masks, np.uint32)
    filters = [int(f) for f in filters]
    assert len(filters) == len(seed_lists)
    lv = np.full((len(seed_lists), n), NOT_WITHIN, np.uint8)
    for f in sorted(set(filters)):
        qs = [q for q, x in enumerate(filters) if x == f]
        lv[qs] = K.levels(n, pairs[(masks & np.uint32(f)) != 0], [seed_lists[q] for q in qs], hops)
    return lv


def type_bits(types):
    """int [r] of row types -> uint32 [r]: 1 << t, 0 for a type outside [0, 32)"""
    t = np.asarray(types, np.int64)
    ok = (t >= 0) & (t < N_TYPES)
    return np.where(ok, np.uint64(1) << np.where(ok, t, 0).astype(np.uint64), 0).astype(np.uint32)


def _allowed(row_masks, filters):
    """bool [B][r]: the row's mask shares a bit with the query's filter"""
    return (np.asarray(row_masks, np.uint32)[None, :] & np.asarray(filters, np.uint32)[:, None]) != 0


def row_levels(lv, relations, row_masks, filters):
    """uint8 [B][r] from the typed dense levels: tests/subgraph_ref.row_levels, 255 where the filter does not hold the row"""
    rl = S.row_levels(lv, relations)
    rl[~_allowed(row_masks, filters)] = NOT_WITHIN
    return rl


def subgraph(n, pairs, masks, seed_lists, filters, hops, relations, row_masks, max_edges):
    """-> (ids, levels, count, level_counts) as tests/subgraph_ref.subgraph"""
    rl = row_levels(levels(n, pairs, masks, seed_lists, filters, hops), relations, row_masks, filters)
    return S.listing(rl, max_edges) + (S.level_counts(rl, hops),)


def paths(n, pairs, masks, sources, source_pairs, f, length):
    """(d, pos) as tests/paths_ref.paths, every source traversed under the one filter f"""
    return P.positions(levels(n, pairs, masks, sources, [f] * len(sources), length), source_pairs, length)


def path_row_levels(pos, relations, row_masks, f):
    """uint8 [np][r]: tests/paths_ref.row_levels, 255 where f does not hold the row"""
    rl = P.row_levels(pos, relations)
    rl[:, (np.asarray(row_masks, np.uint32) & np.uint32(f)) == 0] = P.OFF_PATH
    return rl


def random_typed_graph(n, m, n_types, seed):
    """m random relations (a != b) over n vertices with a type each -> (relations int64 [m][2], types int64 [m]); the input of
    edge_masks.  Duplicates and both orientations occur"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, size=m)
    b = (a + rng.integers(1, n, size=m)) % n
    return np.stack([a, b], axis=1).astype(np.int64), rng.integers(0, n_types, size=m).astype(np.int64)


def random_filters(nq, n_types, seed, allow_empty=False):
    """uint32 [nq] of random filters over the first n_types types, non-empty unless allow_empty"""
    rng = np.random.default_rng(seed)
    f = rng.integers(0 if allow_empty else 1, 1 << n_types, size=nq, dtype=np.uint64)
    return f.astype(np.uint32)
