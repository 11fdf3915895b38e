"""The entity-merging rule of csrc/merge.hip in plain numpy: step 4 of the reference's de-duplication
(Base_Neo4j.py:714-890, _merge_clusters).  Imported by the tests only.

Plan.  labels int64 [n] with values in [0, n), richness integers in [0, 2^32) (all 0 by default).  The primary of a class is its
member of largest richness, among equals the smallest index; primaries are numbered 0 .. n_c - 1 in ascending old index.
Pairs: both ends through new_id, a pair inside one entity dropped (counted, with its weight), the rest (min, max), equal pairs
merged with added weights, ordered by (i, j).  Mentions: entities through new_id, equal (chunk, entity) merged with added
weights, by (chunk, entity).  Relations: rows keep identity and order; a row is dropped iff its ends were different entities of
one class, or an end lies outside [0, n)."""
import numpy as np

MAX_MENTION_WEIGHT = 1 << 12


def sort_reduce(keys, values=None):
    """np.unique + bincount in exact integers -> (distinct keys ascending uint64, sums as Python-int-exact uint64, largest sum)"""
    keys = np.asarray(keys, np.uint64)
    vals = np.ones(len(keys), np.uint64) if values is None else np.asarray(values, np.uint64)
    uniq, inverse = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uniq), np.uint64)
    np.add.at(sums, inverse.ravel(), vals)
    return uniq, sums, int(sums.max()) if len(sums) else 0


def plan(labels, richness=None):
    """-> dict(n, n_merged, primary, new_id, kept, removed), all int64"""
    labels = np.asarray(labels, np.int64)
    n = len(labels)
    rich = np.zeros(n, np.int64) if richness is None else np.asarray(richness, np.int64)
    order = np.lexsort((np.arange(n), -rich, labels))                  # by class, then richness descending, then index ascending
    first = np.ones(n, bool)
    first[1:] = labels[order][1:] != labels[order][:-1]
    best_of_label = np.full(n, -1, np.int64)
    best_of_label[labels[order][first]] = order[first]
    primary = best_of_label[labels]
    is_primary = primary == np.arange(n)
    kept = np.flatnonzero(is_primary).astype(np.int64)
    new_of_kept = np.full(n, -1, np.int64)
    new_of_kept[kept] = np.arange(len(kept))
    return {"n": n, "n_merged": int(len(kept)), "primary": primary, "new_id": new_of_kept[primary], "kept": kept,
            "removed": np.flatnonzero(~is_primary).astype(np.int64)}


def merge_pairs(new_id, pairs, weights=None):
    """-> (pairs int64 [m'][2] by (i, j), weights int64 [m'], dropped pairs, their total weight)"""
    new_id = np.asarray(new_id, np.int64)
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    w = np.ones(len(p), np.int64) if weights is None else np.asarray(weights, np.int64)
    a, b = new_id[p[:, 0]], new_id[p[:, 1]]
    inside = a == b
    lo, hi = np.minimum(a, b)[~inside], np.maximum(a, b)[~inside]
    out, inverse = np.unique(np.stack([lo, hi], axis=1), axis=0, return_inverse=True)
    ws = np.zeros(len(out), np.int64)
    np.add.at(ws, inverse.ravel(), w[~inside])
    return out.reshape(-1, 2), ws, int(inside.sum()), int(w[inside].sum())


def merge_mentions(new_id, n_chunks, mentions, weights=None):
    """(chunk, entity) rows -> (mentions int64 [nnz'][2] by (chunk, entity), weights int64 [nnz'], largest summed weight): the
    list `mention_csr` would be given after relabelling, already merged; a largest weight >= 2^12 is what the device refuses"""
    new_id = np.asarray(new_id, np.int64)
    m = np.asarray(mentions, np.int64).reshape(-1, 2)
    w = np.ones(len(m), np.int64) if weights is None else np.asarray(weights, np.int64)
    out, inverse = np.unique(np.stack([m[:, 0], new_id[m[:, 1]]], axis=1), axis=0, return_inverse=True)
    ws = np.zeros(len(out), np.int64)
    np.add.at(ws, inverse.ravel(), w)
    return out.reshape(-1, 2), ws, int(ws.max()) if len(ws) else 0


def merge_relations(new_id, relations):
    """-> (table int64 [r'][2], row_ids int64 [r'], rows dropped as internal, rows dropped for an end out of range)"""
    new_id = np.asarray(new_id, np.int64)
    n = len(new_id)
    rel = np.asarray(relations, np.int64).reshape(-1, 2)
    ok = (rel >= 0).all(axis=1) & (rel < n).all(axis=1)
    a, b = new_id[np.where(ok, rel[:, 0], 0)], new_id[np.where(ok, rel[:, 1], 0)]
    internal = ok & (rel[:, 0] != rel[:, 1]) & (a == b)
    keep = ok & ~internal
    return np.stack([a[keep], b[keep]], axis=1).reshape(-1, 2), np.flatnonzero(keep).astype(np.int64), int(internal.sum()), int((~ok).sum())


def planted_labels(n, groups, seed):
    """A labelling that merges `groups` disjoint groups of 2 .. 4 random vertices; each group's label is a random member (not the
    smallest), everyone else is a singleton -> int64 [n]"""
    rng = np.random.default_rng(seed)
    labels = np.arange(n, dtype=np.int64)
    perm = rng.permutation(n)
    at = 0
    for _ in range(groups):
        size = int(rng.integers(2, 5))
        if at + size > n:
            break
        members = perm[at:at + size]
        labels[members] = members[int(rng.integers(size))]
        at += size
    return labels
