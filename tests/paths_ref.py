"""The connecting-paths rule of csrc/khop.hip in plain numpy, on top of tests/khop_ref.py: every shortest path of at
most L edges between two sources, MATCH p = allShortestPaths((a)-[*..L]-(b)).  Imported by the tests only.

A source is a seed set as tests/khop_ref.py takes it; hop_s(v) is its k-hop level traversed to depth L.  For a pair p = (A, B) of
source indices, d_p = min over v of hop_A(v) + hop_B(v); where no vertex gives a value <= L, or an index lies outside [0, ns),
d_p = -1 and everything about the pair is empty.  v is on p's paths at position i iff hop_A(v) == i and hop_B(v) == d_p - i; the
dense position of any other vertex is 255.  A row (a, b) of the relation table is at level i + 1 iff one end is at position i and
the other at i + 1; a row between two vertices of one position, a row with a == b and a row with an end outside [0, n) are at no
level (255), and level 0 is empty.  Lists, counts and chunk scores are those of tests/khop_ref.py with positions for hops."""
import numpy as np

from tests import khop_ref as K

OFF_PATH = K.NOT_WITHIN
NO_PATH = -1


def positions(lv, pairs, length):
    """(d int32 [np], pos uint8 [np][n]) from the dense levels uint8 [ns][n] of the sources, traversed to `length`"""
    ns, n = lv.shape
    hop = np.where(lv == K.NOT_WITHIN, 1 << 20, lv.astype(np.int64))
    d = np.full(len(pairs), NO_PATH, np.int32)
    pos = np.full((len(pairs), n), OFF_PATH, np.uint8)
    for p, (ia, ib) in enumerate(pairs):
        if not (0 <= ia < ns and 0 <= ib < ns):
            continue
        both = hop[ia] + hop[ib]
        if both.min() > length:
            continue
        d[p] = both.min()
        on = both == d[p]
        pos[p, on] = lv[ia][on]
    return d, pos


def paths(n, edges, sources, pairs, length):
    """positions for the graph `edges`: (d, pos)"""
    return positions(K.levels(n, edges, sources, length), pairs, length)


def row_levels(pos, relations):
    """uint8 [np][r] from the dense positions uint8 [np][n]: i + 1 for a row that joins positions i and i + 1, else 255"""
    rel = np.asarray(relations, np.int64).reshape(-1, 2)
    n = pos.shape[1]
    ok = (rel >= 0).all(axis=1) & (rel < n).all(axis=1)
    a, b = np.where(ok, rel[:, 0], 0), np.where(ok, rel[:, 1], 0)
    pa, pb = pos[:, a].astype(np.int64), pos[:, b].astype(np.int64)
    on = (pa != OFF_PATH) & (pb != OFF_PATH) & (np.abs(pa - pb) == 1) & ok
    return np.where(on, np.maximum(pa, pb), OFF_PATH).astype(np.uint8)


def counts(x, length):
    """int32 [np][length + 1] from dense positions or row levels"""
    return K.counts(x, length)


def listing(x, cap):
    """(ids int64 [np][cap], positions or levels int32 [np][cap], count int32 [np]) by (position ascending, id ascending)"""
    return K.listing(x, cap)


def chunk_scores(pos, n_chunks, mentions, weights, decay):
    """float64 [np][n_chunks]: tests/khop_ref.chunk_scores with decay by position"""
    return K.chunk_scores(pos, n_chunks, mentions, weights, decay)


def grid_graph(rows, cols):
    """vertex i * cols + j, joined to its right and lower neighbour"""
    e = [(i * cols + j, i * cols + j + 1) for i in range(rows) for j in range(cols - 1)]
    return e + [(i * cols + j, (i + 1) * cols + j) for i in range(rows - 1) for j in range(cols)]


def cycle_graph(n):
    return [(i, (i + 1) % n) for i in range(n)]
