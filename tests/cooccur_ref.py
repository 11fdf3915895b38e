"""The co-occurrence rule of csrc/cooccur.hip in plain Python/numpy.  Imported by the tests only.

Input: a mention CSR by chunk — row_ptr int64 [n_chunks + 1], ent int32 [nnz], w uint32 [nnz] — as rarc_ppr_chunks takes it.  A
row's range is clamped to [0, nnz]; an entry with e outside [0, n) or w outside [1, 2^12) is skipped and counted.  d_c = the valid
entries of chunk c.  A chunk contributes iff 2 <= d_c <= max_mentions; one of more is counted and gives nothing.  A contributing
chunk gives, for every two valid entries at positions i < j with different entities, the pair (min, max) the value 1 ("count") or
w_i * w_j ("product"); two equal entities give nothing.  T = sum d_c (d_c - 1) / 2 over the contributing chunks.  W(a, b) = the
sum of the values of (a, b); an edge exists iff W >= min_weight.  Edges ascend by (a, b)."""
import collections

import numpy as np

MAX_MENTION_WEIGHT = 1 << 12

Result = collections.namedtuple("Result", ("pairs", "weights", "total_pairs", "contributing", "chunks_skipped", "entries_skipped",
                                           "largest_weight", "below_min_weight"))


def csr_of(n_chunks, n, mentions, weights=None):
    """host (chunk, entity) mentions -> (row_ptr, ent, w) as MentionMap stores them: duplicates summed, rows ascending"""
    m = np.asarray(mentions, np.int64).reshape(-1, 2)
    w = np.ones(len(m), np.int64) if weights is None else np.asarray(weights, np.int64)
    acc = {}
    for (c, e), x in zip(m.tolist(), w.tolist()):
        acc[(c, e)] = acc.get((c, e), 0) + x
    keys = sorted(acc)
    row_ptr = np.zeros(n_chunks + 1, np.int64)
    for c, _ in keys:
        row_ptr[c + 1] += 1
    return np.cumsum(row_ptr), np.array([e for _, e in keys], np.int32), np.array([acc[k] for k in keys], np.uint32)


def cooccur(row_ptr, ent, w, n, weight="count", min_weight=1, max_mentions=64):
    """-> Result(pairs int64 [m][2], weights int64 [m], T, contributing chunks, chunks over max_mentions, entries skipped, largest W,
    edges below min_weight)"""
    assert weight in ("count", "product") and min_weight >= 1 and 2 <= max_mentions <= 4096
    row_ptr, ent, w = np.asarray(row_ptr, np.int64), np.asarray(ent, np.int64), np.asarray(w, np.int64)
    nnz = len(ent)
    sums, total, contributing, over, skipped = {}, 0, 0, 0, 0
    for c in range(len(row_ptr) - 1):
        r0 = min(max(int(row_ptr[c]), 0), nnz)
        r1 = min(max(int(row_ptr[c + 1]), r0), nnz)
        row = [(int(ent[i]), int(w[i])) for i in range(r0, r1)]
        valid = [(e, x) for e, x in row if 0 <= e < n and 1 <= x < MAX_MENTION_WEIGHT]
        skipped += len(row) - len(valid)
        d = len(valid)
        if d > max_mentions:
            over += 1
        if not 2 <= d <= max_mentions:
            continue
        contributing += 1
        total += d * (d - 1) // 2
        for i in range(d):
            for j in range(i + 1, d):
                (ea, wa), (eb, wb) = valid[i], valid[j]
                if ea != eb:
                    key = (min(ea, eb), max(ea, eb))
                    sums[key] = sums.get(key, 0) + (1 if weight == "count" else wa * wb)
    keys = sorted(sums)
    kept = [k for k in keys if sums[k] >= min_weight]
    return Result(np.array(kept, np.int64).reshape(-1, 2), np.array([sums[k] for k in kept], np.int64), total, contributing, over, skipped,
                  max(sums.values()) if sums else 0, len(keys) - len(kept))


def cooccur_mentions(n_chunks, n, mentions, weights=None, **kw):
    """the same from host mentions, through csr_of"""
    return cooccur(*csr_of(n_chunks, n, mentions, weights), n, **kw)
