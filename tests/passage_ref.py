"""The passage projection as csrc/ppr.hip defines it, in Python integers — the continuation of tests/ppr_ref.py.

    a mention map: triples (c, e, w), 0 <= c < n_chunks, 0 <= e < n, w an integer >= 1; the weights of a repeated (c, e) add
    up, and every sum stays below 2^12
    S_q(c) = (sum over c's mentions (e, w) of w * p_q(e)) >> 12        (p_q: the PPR state, sum_e p_q(e) <= ONE = 2^40)
    score = S / 2^28 = sum w p / ONE floored to a multiple of 2^-28;  S < 2^40

Every query is projected on its own: a batch is its rows one by one, by construction."""
import random

from tests import ppr_ref as R

WEIGHT_BITS = 12
MAX_WEIGHT = 1 << WEIGHT_BITS          # a summed (chunk, entity) weight stays below this
SCORE_ONE = 1 << 28


def merged(n_chunks, n, mentions, weights=None):
    """{(c, e): w} with the weights of duplicates added"""
    out = {}
    for i, (c, e) in enumerate(mentions):
        w = 1 if weights is None else int(weights[i])
        assert 0 <= c < n_chunks and 0 <= e < n and w >= 1
        out[(c, e)] = out.get((c, e), 0) + w
    assert all(w < MAX_WEIGHT for w in out.values())
    return out


def raw_sums(p, n_chunks, mentions, weights=None):
    """sum w * p per chunk, before the shift"""
    acc = [0] * n_chunks
    for (c, e), w in merged(n_chunks, len(p), mentions, weights).items():
        acc[c] += w * p[e]
    return acc


def chunk_state(p, n_chunks, mentions, weights=None):
    """S for one query's state p (a list of n integers)"""
    return [x >> WEIGHT_BITS for x in raw_sums(p, n_chunks, mentions, weights)]


def chunk_states_batch(states, n_chunks, mentions, weights=None):
    """`chunk_state` for every row of a uint64 [B][n] array of states at once, in numpy uint64 -> uint64 [B][n_chunks].  The
    Python-integer functions above stay the definition (tests/test_ppr_batch_ref_host.py finds this one equal to them); the
    sums are asserted below 2^63 (csrc/ppr.hip proves 2^52)."""
    import numpy as np

    states = np.asarray(states, dtype=np.uint64)
    items = sorted(merged(n_chunks, states.shape[1], mentions, weights).items())
    c = np.asarray([k[0] for k, _ in items], dtype=np.int64)
    e = np.asarray([k[1] for k, _ in items], dtype=np.int64)
    w = np.asarray([x for _, x in items], dtype=np.uint64)
    terms = states[:, e] * w[None, :]                                     # w p < 2^12 * 2^40
    assert int(states.max()) <= R.ONE and int(terms.max()) < 1 << 63
    acc = np.zeros((states.shape[0], n_chunks), np.uint64)
    np.add.at(acc, (np.arange(states.shape[0])[:, None], c[None, :]), terms)
    assert int(acc.max()) < 1 << 63
    return acc >> np.uint64(WEIGHT_BITS)


def scores(S):
    """S / 2^28 as floats: exact, S < 2^40 < 2^53"""
    return [x / SCORE_ONE for x in S]


def topk(S, k):
    """(ids, scores, count): the chunks of positive score by (score descending, chunk ascending), cut at k, (-1, -inf) behind"""
    order = sorted((c for c in range(len(S)) if S[c] > 0), key=lambda c: (-S[c], c))[:k]
    pad = k - len(order)
    return order + [-1] * pad, [S[c] / SCORE_ONE for c in order] + [float("-inf")] * pad, len(order)


# ---- mention maps ------------------------------------------------------------------------------------------------------------------
def chunk_of_degree(n, d, seed, chunk=0, max_weight=MAX_WEIGHT - 1):
    """`d` mentions of distinct entities for one chunk -> (mentions, weights)"""
    rng = random.Random(seed)
    ents = rng.sample(range(n), d)
    return [(chunk, e) for e in ents], [rng.randint(1, max_weight) for _ in ents]


def random_mentions(n, n_chunks, seed, max_degree=12, max_weight=MAX_WEIGHT - 1):
    """every chunk mentions 0 .. max_degree distinct entities -> (mentions, weights), shuffled"""
    rng = random.Random(seed)
    mentions, weights = [], []
    for c in range(n_chunks):
        for e in rng.sample(range(n), rng.randint(0, max_degree)):
            mentions.append((c, e))
            weights.append(rng.randint(1, max_weight))
    order = list(range(len(mentions)))
    rng.shuffle(order)
    return [mentions[i] for i in order], [weights[i] for i in order]


def with_twins(mentions, weights, src, dst):
    """chunk `dst` (without mentions so far) gets exactly the mentions of chunk `src`"""
    assert not any(c == dst for c, _ in mentions)
    extra = [(i, e) for i, (c, e) in enumerate(mentions) if c == src]
    return mentions + [(dst, e) for _, e in extra], weights + [weights[i] for i, _ in extra]


def split_weights(mentions, weights, seed):
    """every weight >= 2 split over two duplicates of its (chunk, entity); then shuffled"""
    rng = random.Random(seed)
    m2, w2 = [], []
    for (c, e), w in zip(mentions, weights):
        if w >= 2:
            a = rng.randint(1, w - 1)
            m2 += [(c, e), (c, e)]
            w2 += [a, w - a]
        else:
            m2.append((c, e))
            w2.append(w)
    order = list(range(len(m2)))
    rng.shuffle(order)
    return [m2[i] for i in order], [w2[i] for i in order]


__all__ = ["R", "chunk_state", "chunk_states_batch", "scores", "topk", "raw_sums", "merged", "chunk_of_degree", "random_mentions", "with_twins", "split_weights"]
