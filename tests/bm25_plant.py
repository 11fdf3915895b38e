"""Planted BM25 indexes for the selection and merge kernels of csrc/bm25.hip (imported by tests only).

`plant(n_docs, vectors, idf)` builds the arrays of a `Bm25Index` from score vectors: term t has a posting for every document
with S_t[d] != 0, post_w = S_t[d].  With idf[t] = 1.0 a one-token query scores exactly S_t[d] (0.0 + 1.0 * w is exact), so a
test decides the bits of every score, where they lie in the 8192-document tiles, and which merge group sees them.

The reference is written here and does not use the project's `topk_order`: scores are accumulated one token after another
in float64, in query order (`ref_scores`); the order is a full stable sort, score descending then id ascending
(`ref_order`).  `rounds`, `tile_of` and `group_of` restate the launch plan of rarc_bm25_topk: tiles of T documents, merge
groups of T // k candidate lists, rounds until one group holds every list.

`BUILDERS` is the catalogue the GPU file runs and tests/test_bm25_plant_host.py proves, case by case, to be what its name says.
"""
import functools
import itertools

import numpy as np

from rag_arc_amd.hip import bm25 as M
from rag_arc_amd.hip.bm25 import Bm25Index

T = 8192                     # BM_T: documents per tile, items per merge workgroup
assert M.MAX_DOCS == 0x7fffffff - T and M.MAX_K == 1024, "csrc/bm25.hip's tile size or k limit changed: revisit every case"
MAX_K = 1024

DBL_MAX = float(np.finfo(np.float64).max)
MIN_NORMAL = float(np.finfo(np.float64).tiny)
MIN_SUB = 5e-324


# -- the launch plan -----------------------------------------------------------------------------------------------------
def tiles(n_docs):
    return (n_docs + T - 1) // T


def rounds(n_docs, k):
    """Candidate lists entering each merge round, the final one included: [65, 9, 2] for 65 tiles at k = 1024."""
    group = T // k
    out = [tiles(n_docs)]
    while out[-1] > group:
        out.append((out[-1] + group - 1) // group)
    return out


def tile_of(doc):
    return np.asarray(doc) // T


def group_of(doc, k, rnd=0):
    """The merge workgroup of round `rnd` (0 = first) that sees document `doc`'s candidate."""
    return np.asarray(doc) // T // (T // k) ** (rnd + 1)


# -- the planted index and its reference -----------------------------------------------------------------------------------
def plant(n_docs, vectors, idf=None):
    """A Bm25Index whose term t scores S_t = vectors[t]; idf defaults to 1.0 for every term."""
    vectors = [np.asarray(v, dtype=np.float64) for v in vectors]
    assert vectors and all(v.shape == (n_docs,) for v in vectors)
    idf = np.ones(len(vectors)) if idf is None else np.asarray(idf, dtype=np.float64)
    assert idf.shape == (len(vectors),)
    docs = [np.flatnonzero(v != 0) for v in vectors]
    post_off = np.zeros(len(vectors) + 1, dtype=np.int64)
    np.cumsum([d.size for d in docs], out=post_off[1:])
    post_doc = np.concatenate(docs).astype(np.int32)
    post_w = np.concatenate([v[d] for v, d in zip(vectors, docs)])
    present = np.diff(post_off) > 0
    return Bm25Index(post_off, post_doc, post_w, idf.copy(), present, np.ones(n_docs, dtype=np.int64), 1.0,
                     float(idf.mean()), 1.5, 0.75, 0.25)


def ref_scores(n_docs, vectors, idf, query):
    """score[d] = (((0.0 + idf[t0] * S_t0[d]) + idf[t1] * S_t1[d]) + ...), tokens in query order, float64; a document a
    token does not reach is left alone (the scorer adds an exact zero there)."""
    score = np.zeros(n_docs, dtype=np.float64)
    for t in query:
        s = vectors[t]
        d = np.flatnonzero(s != 0)
        score[d] = score[d] + np.float64(idf[t]) * s[d]
    return score


def ref_order(scores, k):
    return np.lexsort((np.arange(scores.size), -scores))[:k]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def cut(scores, k):
    """(inside, outside): how many documents equal to the k-th best score the top k takes, and how many it leaves.
    outside == 0 is the final select's exact exit; otherwise it bisects over the id."""
    order = ref_order(scores, scores.size)
    s = scores[order]
    eq = np.flatnonzero(s == s[k - 1])
    return int((eq < k).sum()), int((eq >= k).sum())


class Case:
    """One planted index, its queries, and the k values to ask for."""

    def __init__(self, n_docs, vectors, queries, ks, idf=None):
        self.n_docs, self.queries, self.ks = int(n_docs), [list(q) for q in queries], tuple(ks)
        self.vectors = [np.asarray(v, dtype=np.float64) for v in vectors]
        self.idf = np.ones(len(self.vectors)) if idf is None else np.asarray(idf, dtype=np.float64)
        self._scores = {}

    def index(self):
        return plant(self.n_docs, self.vectors, self.idf)

    def scores(self, q):
        """Reference scores of query number q: computed once, read-only."""
        if q not in self._scores:
            s = ref_scores(self.n_docs, self.vectors, self.idf, self.queries[q])
            s.setflags(write=False)
            self._scores[q] = s
        return self._scores[q]

    def order(self, q, k):
        return ref_order(self.scores(q), k)


# -- merge depth -------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = {"8T": 8 * T, "8T+1": 8 * T + 1, "64T": 64 * T, "65T-5": 65 * T - 5}
MERGE_KS = (1024, 1000, 683, 3, 1)
Q_LAST, Q_ROBIN, Q_EMPTY = 0, 1, 2


def winner_value(rank):
    return 1.0 + 0.5 * (MAX_K - rank)          # rank 0 is the best; distinct, exact


def merge_depth(n_docs):
    """Term 0: the 1024 winners are the last 1024 documents, the best of all the very last one.  Term 1: the winner of
    rank r lies in tile r mod n_tiles.  A few negatives lie in every tile.  The third query is empty."""
    rng = np.random.default_rng(n_docs)
    nt = tiles(n_docs)
    ranks = rng.permutation(MAX_K)
    j = int(np.flatnonzero(ranks == 0)[0])
    ranks[j], ranks[-1] = ranks[-1], 0
    last = np.zeros(n_docs)
    last[n_docs - MAX_K:] = winner_value(ranks)
    robin = np.zeros(n_docs)
    for r in range(MAX_K):
        tile = r % nt
        n_here = min(T, n_docs - tile * T)
        d = tile * T + ((r // nt) * 7 + 3) % n_here
        if robin[d] == 0:                       # a one-document tile holds one winner only
            robin[d] = winner_value(r)
    neg = np.arange(5, n_docs, 1013)
    for v in (last, robin):
        at = neg[v[neg] == 0]
        v[at] = -(1.0 + at % 5)
    return Case(n_docs, [last, robin], [[0], [1], []], MERGE_KS)


# -- ties at the cut -----------------------------------------------------------------------------------------------------------
TIE_N = 65 * T
TIE_TOP = 64 * T + np.array([100, 200, 300])            # three documents above the tie, in the last tile
TIE_DOCS = np.sort(np.concatenate([np.arange(65) * T, np.arange(65) * T + T - 1]))
TIE_KS = {"inside_tile": 14, "tile_edge": 15, "group_edge": 129}
Q_TIED, Q_UNIQUE = 0, 1


def ties(v):
    """v on slots 0 and 8191 of all 65 tiles (130 documents) under three better documents in the last tile.  v > 0: every
    other document is untouched (0.0) and ranks below.  v < 0: the three better documents are the untouched ones and every
    other document scores below v.  Term 1 is the same with the 130 values made distinct, descending with the id."""
    if v > 0:
        base = np.zeros(TIE_N)
        top = v + 1.0 + np.arange(3)
    else:
        base = 1000.0 * v - (np.arange(TIE_N) % 97)
        top = np.zeros(3)
    tied, unique = base.copy(), base.copy()
    tied[TIE_DOCS] = v
    unique[TIE_DOCS] = v + (TIE_DOCS.size - np.arange(TIE_DOCS.size)) * 2.0 ** -30
    tied[TIE_TOP] = unique[TIE_TOP] = top
    return Case(TIE_N, [tied, unique], [[0], [1], []], tuple(TIE_KS.values()))


# -- all equal ---------------------------------------------------------------------------------------------------------------
def all_equal(n_docs, ks):
    return Case(n_docs, [np.full(n_docs, 2.5), np.full(n_docs, -2.5)], [[0], [1], []], ks)


# -- short last tile -----------------------------------------------------------------------------------------------------------
SHORT_KS = (100, 1024)
Q_TOP, Q_BOTTOM, Q_TOP_BELOW_ZERO = 0, 1, 2


def short_r(k):
    return (1, 5, k - 1, k, k + 1)


def short_tile(r, k):
    """T + r documents.  Tile 0 holds distinct scores in [1, 2).  Term 0: the r last documents hold the top scores;
    term 1: they hold the lowest.  Term 2 is term 0 moved below zero: every score is negative, in the same order.  For
    r < k the last tile's list then holds real negative scores beside placeholder slots (key 1), and the negative scores
    must win.  Terms 0 and 1 cannot show a placeholder that ranks as 0.0: tile 0 alone outranks it."""
    n = T + r
    body = 1.0 + (np.arange(T) * 7919 % T) / T
    tail = np.random.default_rng(r * 2048 + k).permutation(r) + 10.0
    top = np.concatenate([body, tail])
    return Case(n, [top, np.concatenate([body, -tail]), top - 4096.0], [[0], [1], [2], []], (k,))


def small_corpus(n_docs, ks):
    s = np.random.default_rng(n_docs).permutation(n_docs) - (n_docs // 2) + 0.5      # distinct, both signs
    return Case(n_docs, [s], [[0], []], ks)


# -- key order -----------------------------------------------------------------------------------------------------------------
RUN = 2000
KEY_UNTOUCHED = 5
KEY_ABOVE_RUN = 6 + KEY_UNTOUCHED + 2          # six positive specials, the untouched documents, -MIN_SUB, -MIN_NORMAL
KEY_KS = (1, 7, KEY_ABOVE_RUN + 500, 1024)


def special_values():
    one = [1.0, float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0))]
    pos = [DBL_MAX, MIN_SUB, MIN_NORMAL] + one
    return np.array(pos + [-x for x in pos])


def consecutive_run():
    """2000 consecutive doubles around -1e-300."""
    mid = int(np.array([-1e-300]).view(np.int64)[0])
    return np.arange(mid - RUN // 2, mid + RUN // 2, dtype=np.int64).view(np.float64).copy()


def key_order(n_docs):
    """The special values and the run scattered over the corpus, five documents untouched, every other document below
    the run (-1e-290 and lower) and above -1 - 2^-52."""
    rng = np.random.default_rng(n_docs)
    values = np.concatenate([special_values(), consecutive_run(), np.zeros(KEY_UNTOUCHED)])
    s = -1e-290 * (1.0 + rng.integers(0, 4000, size=n_docs))
    s[rng.permutation(n_docs)[:values.size]] = values
    return Case(n_docs, [s], [[0], []], KEY_KS)


# -- summation order -------------------------------------------------------------------------------------------------------------
SUM_N = 2 * T + 77
SUM_K = 100


def summation_order():
    """Terms 0-2: weights a, b, -a with a a multiple of 1e16 and b in {1, 2, 3}, idf 1.  Terms 3-5: a, b, a with idf
    1, 1, -1.  Terms 6-8: random weights and idfs (every product rounds).  Some documents lack one or two of a triple."""
    rng = np.random.default_rng(16)
    d = np.arange(SUM_N)
    a = 1e16 * (1 + d % 5)
    b = 1.0 + d % 3
    has = [d % 7 != 0, d % 11 != 0, d % 13 != 0]
    vec = [np.where(has[0], a, 0.0), np.where(has[1], b, 0.0), np.where(has[2], -a, 0.0)]
    vec += [vec[0].copy(), vec[1].copy(), np.where(has[2], a, 0.0)]
    vec += [np.where(rng.random(SUM_N) < 0.8, rng.standard_normal(SUM_N), 0.0) for _ in range(3)]
    idf = np.array([1.0, 1.0, 1.0, 1.0, 1.0, -1.0] + rng.uniform(-2.0, 3.0, size=3).tolist())
    queries = [list(p) for t0 in (0, 3, 6) for p in itertools.permutations(range(t0, t0 + 3))]
    queries += [[0, 0, 1], [0, 1, 0], [3, 5, 5, 4], [6, 7, 6, 8, 7], []]
    return Case(SUM_N, vec, queries, (SUM_K,), idf)


# -- long posting runs -------------------------------------------------------------------------------------------------------------
LONG_N = 3 * T - 9
LONG_K = 1000


def long_runs():
    """Term 0 in every document: 8192 postings in tiles 0 and 1 (four full trips of the four-in-flight loop), 8183 in the
    last.  Term 1 in 2049 documents of tile 1: one full trip and a remainder trip of one posting."""
    rng = np.random.default_rng(25)
    every = rng.uniform(0.5, 3.0, size=LONG_N)
    some = np.zeros(LONG_N)
    some[T + np.sort(rng.permutation(T)[:2049])] = rng.uniform(0.5, 3.0, size=2049)
    return Case(LONG_N, [every, some], [[0, 1], [1, 0], [1], [0], [1, 1, 0], []], (LONG_K,), np.array([0.7, -1.3]))


# -- the catalogue ---------------------------------------------------------------------------------------------------------------
BUILDERS = {}
for _name, _n in MERGE_SHAPES.items():
    BUILDERS[f"merge_{_name}"] = (merge_depth, (_n,), MERGE_KS)
BUILDERS["ties_pos"] = (ties, (2.5,), tuple(TIE_KS.values()))
BUILDERS["ties_neg"] = (ties, (-2.5,), tuple(TIE_KS.values()))
BUILDERS["equal_T"] = (all_equal, (T, (1, 100, 1024)), (1, 100, 1024))
BUILDERS["equal_8T"] = (all_equal, (8 * T, (1024,)), (1024,))
for _k in SHORT_KS:
    for _r in short_r(_k):
        BUILDERS[f"short_T+{_r}_k{_k}"] = (short_tile, (_r, _k), (_k,))
BUILDERS["small_1024"] = (small_corpus, (1024, (1024, 1)), (1024, 1))
BUILDERS["small_1"] = (small_corpus, (1, (1,)), (1,))
BUILDERS["small_T"] = (small_corpus, (T, (1024, 100, 1)), (1024, 100, 1))
BUILDERS["small_T+1"] = (small_corpus, (T + 1, (1024, 100, 1)), (1024, 100, 1))
BUILDERS["keys_T"] = (key_order, (T,), KEY_KS)
BUILDERS["keys_3T"] = (key_order, (3 * T - 100,), KEY_KS)
BUILDERS["sum_order"] = (summation_order, (), (SUM_K,))
BUILDERS["long_runs"] = (long_runs, (), (LONG_K,))

CASE_KS = [(name, k) for name, (_, _, ks) in BUILDERS.items() for k in ks]


@functools.lru_cache(maxsize=None)
def case(name):
    fn, args, ks = BUILDERS[name]
    c = fn(*args)
    assert c.ks == tuple(ks), name
    for v in c.vectors:
        v.setflags(write=False)
    return c
