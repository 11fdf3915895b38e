"""The k-hop neighbourhood rule of csrc/khop.hip in plain Python / numpy: levels, counts, list, chunk scores.
Imported by the tests only.

Edge weights are ignored.  hop_q(v) = the fewest edges from any seed of q to v (a seed has hop 0); v is in the neighbourhood
iff hop_q(v) <= hops; the dense level of any other vertex is 255.  The list is ordered by (hop ascending, vertex ascending) and
cut at max_vertices, (-1, -1) behind; counts[h] is never cut.  Chunks: S(c) = sum over c's mentions (e, w) with hop(e) <= hops
of w * decay[hop(e)], score S / 2^28."""
import numpy as np

from tests import passage_ref as P
from tests.ppr_ref import path_graph, random_graph, star_graph, two_components_and_isolated  # noqa: F401  (the graphs of the PPR tests)

NOT_WITHIN = 255
MAX_HOPS = 8
SCORE_ONE = 1 << 28


def neighbours(n, edges):
    adj = [[] for _ in range(n)]
    for i, j in edges:
        adj[i].append(j)
        adj[j].append(i)
    return adj


def levels_one(n, edges, seeds, hops, adj=None):
    """uint8 [n]: the hop of every vertex from the seeds (-1 and out-of-range slots are unused), 255 beyond `hops`"""
    adj = neighbours(n, edges) if adj is None else adj
    lv = np.full(n, NOT_WITHIN, np.uint8)
    frontier = sorted({int(v) for v in seeds if 0 <= int(v) < n})
    for v in frontier:
        lv[v] = 0
    for h in range(1, hops + 1):
        nxt = set()
        for u in frontier:
            for v in adj[u]:
                if lv[v] == NOT_WITHIN:
                    nxt.add(v)
        for v in nxt:
            lv[v] = h
        frontier = sorted(nxt)
    return lv


def levels(n, edges, seed_lists, hops):
    """uint8 [B][n]: levels_one for every row, as one frontier matrix per hop (tests/test_khop_ref_host.py holds the two equal)"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    order = np.argsort(dst, kind="stable")
    src, dst = src[order], dst[order]
    starts = np.flatnonzero(np.r_[True, dst[1:] != dst[:-1]]) if dst.size else np.zeros(0, np.int64)
    heads = dst[starts]
    lv = np.full((len(seed_lists), n), NOT_WITHIN, np.uint8)
    for q, s in enumerate(seed_lists):
        for v in s:
            if 0 <= int(v) < n:
                lv[q, int(v)] = 0
    frontier = lv == 0
    for h in range(1, hops + 1):
        if not frontier.any():
            break
        reach = np.zeros(lv.shape, bool)
        if starts.size:
            reach[:, heads] = np.logical_or.reduceat(frontier[:, src], starts, axis=1)
        frontier = reach & (lv == NOT_WITHIN)
        lv[frontier] = h
    return lv


def counts(lv, hops):
    """int32 [B][hops + 1] from the dense levels"""
    return np.stack([(lv == h).sum(axis=1) for h in range(hops + 1)], axis=1).astype(np.int32)


def listing(lv, max_vertices):
    """(ids int64 [B][max], hops int32 [B][max], count int32 [B]) from the dense levels"""
    B = lv.shape[0]
    ids = np.full((B, max_vertices), -1, np.int64)
    hp = np.full((B, max_vertices), -1, np.int32)
    cnt = np.zeros(B, np.int32)
    for q in range(B):
        inside = np.flatnonzero(lv[q] != NOT_WITHIN)
        order = inside[np.lexsort((inside, lv[q][inside]))][:max_vertices]
        ids[q, :order.size], hp[q, :order.size], cnt[q] = order, lv[q][order], order.size
    return ids, hp, cnt


def default_decay(hops):
    return [4096 >> (2 * h) for h in range(hops + 1)]


def chunk_state(lv_row, n_chunks, mentions, weights, decay):
    """S for one query's dense levels, as Python integers; duplicates of a (chunk, entity) merged as MentionMap merges them"""
    acc = [0] * n_chunks
    for (c, e), w in P.merged(n_chunks, len(lv_row), mentions, weights).items():
        if lv_row[e] != NOT_WITHIN:
            acc[c] += w * int(decay[int(lv_row[e])])
    assert all(0 <= x < SCORE_ONE for x in acc)
    return acc


def chunk_scores(lv, n_chunks, mentions, weights, decay):
    """float64 [B][n_chunks] = S / 2^28, exact: chunk_state for every row, as one table look-up (S < 2^28: float64 sums are exact)"""
    merged = P.merged(n_chunks, lv.shape[1], mentions, weights)
    c = np.array([k[0] for k in merged], np.int64)
    e = np.array([k[1] for k in merged], np.int64)
    w = np.array(list(merged.values()), np.float64)
    table = np.zeros(256, np.float64)
    table[:len(decay)] = decay
    out = np.zeros((lv.shape[0], n_chunks), np.float64)
    for q in range(lv.shape[0]):
        out[q] = np.bincount(c, weights=w * table[lv[q][e]], minlength=n_chunks)
    assert out.max(initial=0) < SCORE_ONE
    return out / SCORE_ONE


def chunk_topk(S, k):
    """as tests/passage_ref.topk: positive scores by (score descending, chunk ascending), cut at k, (-1, -inf) behind"""
    return P.topk(S, k)


def random_seeds(n, nq, n_slots, seed):
    """nq rows of 0 .. n_slots seeds (four rows in five full, the first among them), some repeated"""
    rng = np.random.default_rng(seed)
    rows = []
    for q in range(nq):
        k = n_slots if q % 5 != 4 else int(rng.integers(0, n_slots + 1))
        rows.append([int(v) for v in rng.integers(0, n, size=k)])
    return rows
