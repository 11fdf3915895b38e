"""Typed personalized PageRank as csrc/ppr.hip defines it, by composition of two references that stand on their
own: tests/typed_ref.py's mask test picks the edges a query may cross, tests/ppr_ref.py runs the integer rule on them.

    query q carries a filter F_q (a uint32); its graph holds the pairs with mask & F_q != 0, each at its full weight
    W_q(u) = the sum of the weights of u's pairs in that graph;  c(u) = p(u) // W_q(u)
    flow(v) = sum over v's pairs {u, v} in that graph of w_uv * c(u)   (W_q(v) = 0: flow(v) = p(v))
    p', delta, freezing, scores and ranking exactly as tests/ppr_ref.py

Nothing here knows how the kernels get there (a second accumulator in the step): a query is filtered, then ranked alone."""
import numpy as np

from tests import passage_ref as C
from tests import ppr_ref as R
from tests import typed_ref as T

ALL = T.ALL
ONE = R.ONE


def filtered(pairs, masks, weights, f):
    """the pair list query filter f crosses -> (edges as a list of tuples, their weights or None)"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    keep = (np.asarray(masks, np.uint32) & np.uint32(int(f))) != 0          # typed_ref's test: the mask shares a bit with the filter
    edges = [tuple(e) for e in pairs[keep].tolist()]
    return edges, None if weights is None else [int(w) for w in np.asarray(weights)[keep]]


def ppr_one(n, pairs, masks, seeds, f, seed_weights=None, weights=None, **kw):
    """one query under filter f -> (p as a list of n Python integers, iterations run)"""
    edges, w = filtered(pairs, masks, weights, f)
    return R.ppr_one(n, edges, seeds, seed_weights, weights=w, **kw)


def ppr_batch(n, pairs, masks, seed_lists, filters, seed_weight_lists=None, weights=None, **kw):
    """a batch of mixed filters -> (uint64 [B][n], list of iterations run): the queries of one filter share a filtered pair list
    and one tests/ppr_ref.ppr_batch call (which tests/test_ppr_batch_ref_host.py finds equal to ppr_one row for row)"""
    filters = [int(f) for f in filters]
    assert len(filters) == len(seed_lists)
    out = np.zeros((len(seed_lists), n), np.uint64)
    its = [0] * len(seed_lists)
    for f in sorted(set(filters)):
        qs = [q for q, x in enumerate(filters) if x == f]
        edges, w = filtered(pairs, masks, weights, f)
        sw = None if seed_weight_lists is None else [seed_weight_lists[q] for q in qs]
        p, it = R.ppr_batch(n, edges, [seed_lists[q] for q in qs], sw, weights=w, **kw)
        out[qs] = p
        for i, q in enumerate(qs):
            its[q] = it[i]
    return out, its


def chunk_states(states, n_chunks, mentions, mention_weights=None):
    """the passage projection of a typed batch: tests/passage_ref's, which reads a state whatever produced it"""
    return C.chunk_states_batch(states, n_chunks, mentions, mention_weights)


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
def random_typed_weighted(n, m, n_types, seed, max_weight=7):
    """m distinct random pairs i < j, each with a random non-empty multi-bit mask over n_types types and a weight in
    1 .. max_weight -> (pairs as a list of tuples, masks uint32 [m], weights as a list)"""
    edges, weights = R.random_graph(n, m, seed, max_weight=max_weight)
    masks = T.random_filters(len(edges), n_types, seed + 1)
    return edges, masks, weights


def with_typed_hub(n, edges, masks, weights, d, n_types, max_weight=7):
    """one more vertex, n, joined to 0 .. d - 1; the type of the edge to v is v % n_types, its weight 1 + v % max_weight"""
    edges = list(edges) + [(v, n) for v in range(d)]
    masks = np.concatenate([np.asarray(masks, np.uint32), np.array([1 << (v % n_types) for v in range(d)], np.uint32)])
    return n + 1, edges, masks, list(weights) + [1 + v % max_weight for v in range(d)]


def allowed_degrees(n, edges, masks, f):
    """the number of neighbours of every vertex that filter f lets it reach"""
    return R.degrees(n, filtered(edges, masks, None, f)[0])
