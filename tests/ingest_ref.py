"""The graph-ingest rule of csrc/merge.hip in plain Python dicts and loops.  Imported by the tests only.

Pairs.  n vertices; r new rows (a, b) in any orientation, each with an optional weight and an optional type; optionally a base: m0
unique pairs i < j in any order with optional weights and optional type masks.  A new row is skipped and counted under the FIRST
that applies of: an end outside [0, n) / a == b / weight 0 / a type outside [0, 32).  A base row outside its contract (i >= j, out
of range, weight 0) is skipped and counted apart.  Every other row gives its weight to the pair (min, max) and its mask (1 << type;
a base row's whole mask) to the pair's mask.  W = the sum, mask = the OR.  Unit mode — neither side has weights — makes every W 1;
when only one side has weights the other side's rows count 1 each.  Edges ascend by (i, j).

Mentions.  r new rows (chunk, entity) with optional weights; optionally a base CSR.  A row is skipped and counted under the first
of: chunk outside [0, n_chunks) / entity outside [0, n_entities) / weight outside [1, 2^12).  W(c, e) = the sum of the weights; the
output is the CSR mention_csr produces and the list of chunks of more than split_degree mentions."""
import collections

import numpy as np

MAX_MENTION_WEIGHT = 1 << 12
N_TYPES = 32

Pairs = collections.namedtuple("Pairs", ("pairs", "weights", "masks", "edges", "largest", "total", "skipped", "base_skipped"))
Mentions = collections.namedtuple("Mentions", ("row_ptr", "entities", "weights", "split", "nnz", "largest", "skipped", "base_skipped"))

PAIR_KINDS = ("out_of_range", "self_loop", "zero_weight", "bad_type")
MENTION_KINDS = ("chunk_out_of_range", "entity_out_of_range", "bad_weight")


def _list(x):
    return None if x is None else [int(v) for v in np.asarray(x).reshape(-1).tolist()]


def ingest_pairs(n, rows, weights=None, types=None, base_pairs=None, base_weights=None, base_masks=None):
    """-> Pairs(pairs int64 [m][2], weights uint64 [m] or None (unit mode), masks uint32 [m] or None (untyped), edges, largest W,
    total W, skipped {kind: count}, base rows skipped)"""
    rows = [(int(a), int(b)) for a, b in np.asarray(rows, np.int64).reshape(-1, 2).tolist()]
    base = [] if base_pairs is None else [(int(a), int(b)) for a, b in np.asarray(base_pairs, np.int64).reshape(-1, 2).tolist()]
    weights, types, base_weights, base_masks = _list(weights), _list(types), _list(base_weights), _list(base_masks)
    typed = types is not None or base_masks is not None
    if typed:
        assert (types is not None or not rows) and (base_masks is not None or not base), "typed and untyped inputs are mixed"
    unit = weights is None and base_weights is None
    skipped = dict.fromkeys(PAIR_KINDS, 0)
    base_skipped = 0
    weight_of, mask_of = {}, {}

    def give(a, b, w, mask):
        key = (min(a, b), max(a, b))
        weight_of[key] = weight_of.get(key, 0) + w
        mask_of[key] = mask_of.get(key, 0) | mask

    for i, (a, b) in enumerate(base):
        w = 1 if base_weights is None else base_weights[i]
        if not (0 <= a < b < n) or w == 0:
            base_skipped += 1
            continue
        give(a, b, w, base_masks[i] if base_masks is not None else 0)
    for i, (a, b) in enumerate(rows):
        w = 1 if weights is None else weights[i]
        t = 0 if types is None else types[i]
        if not (0 <= a < n and 0 <= b < n):
            skipped["out_of_range"] += 1
        elif a == b:
            skipped["self_loop"] += 1
        elif w == 0:
            skipped["zero_weight"] += 1
        elif not 0 <= t < N_TYPES:
            skipped["bad_type"] += 1
        else:
            give(a, b, w, 1 << t)
    keys = sorted(weight_of)
    w_out = [1 if unit else weight_of[k] for k in keys]
    return Pairs(np.array(keys, np.int64).reshape(-1, 2), None if unit else np.array(w_out, np.uint64),
                 np.array([mask_of[k] for k in keys], np.uint32) if typed else None, len(keys), max(w_out) if keys else 0, sum(w_out), skipped,
                 base_skipped)


def expand_base(base_pairs, base_weights=None, base_masks=None):
    """A base as rows: an edge with a multi-bit mask becomes one row per bit, the weight on the first and 0 on the others -> (rows,
    weights or None, types or None).  The host constructor refuses a weight of 0, so a caller that compares against it hands it
    the masks through all rows without weights, and the weights through the rows of non-zero weight without types."""
    rows, ws, ts = [], [], []
    base_pairs = np.asarray(base_pairs, np.int64).reshape(-1, 2).tolist()
    for i, (a, b) in enumerate(base_pairs):
        w = 1 if base_weights is None else int(base_weights[i])
        if base_masks is None:
            rows.append((a, b)), ws.append(w)
            continue
        bits = [t for t in range(N_TYPES) if (int(base_masks[i]) >> t) & 1]
        for j, t in enumerate(bits):
            rows.append((a, b)), ts.append(t)
            ws.append(w if j == 0 else 0)
    return np.array(rows, np.int64).reshape(-1, 2), (None if base_weights is None else np.array(ws, np.int64)), (np.array(ts, np.int64) if base_masks is not None else None)


def ingest_mentions(n_chunks, n_entities, rows, weights=None, base=None, split_degree=64):
    """base: None or (row_ptr, entities, weights) of a CSR over its own (fewer or equal) chunks.
    -> Mentions(row_ptr int64 [n_chunks + 1], entities int32 [nnz], weights uint64 [nnz], split int32, nnz, largest W,
    skipped {kind: count}, base entries skipped)"""
    rows = [(int(c), int(e)) for c, e in np.asarray(rows, np.int64).reshape(-1, 2).tolist()]
    weights = _list(weights)
    skipped = dict.fromkeys(MENTION_KINDS, 0)
    base_skipped = 0
    acc = {}
    if base is not None:
        row_ptr, ent, w = (_list(x) for x in base)
        nnz0 = len(ent)
        for c in range(len(row_ptr) - 1):
            r0 = min(max(row_ptr[c], 0), nnz0)
            r1 = min(max(row_ptr[c + 1], r0), nnz0)
            for i in range(r0, r1):
                if 0 <= ent[i] < n_entities and 1 <= w[i] < MAX_MENTION_WEIGHT and c < n_chunks:
                    acc[(c, ent[i])] = acc.get((c, ent[i]), 0) + w[i]
                else:
                    base_skipped += 1
    for i, (c, e) in enumerate(rows):
        w = 1 if weights is None else weights[i]
        if not 0 <= c < n_chunks:
            skipped["chunk_out_of_range"] += 1
        elif not 0 <= e < n_entities:
            skipped["entity_out_of_range"] += 1
        elif not 1 <= w < MAX_MENTION_WEIGHT:
            skipped["bad_weight"] += 1
        else:
            acc[(c, e)] = acc.get((c, e), 0) + w
    keys = sorted(acc)
    degree = [0] * n_chunks
    for c, _ in keys:
        degree[c] += 1
    row_ptr = [0]
    for d in degree:
        row_ptr.append(row_ptr[-1] + d)
    return Mentions(np.array(row_ptr, np.int64), np.array([e for _, e in keys], np.int32), np.array([acc[k] for k in keys], np.uint64),
                    np.array([c for c in range(n_chunks) if degree[c] > split_degree], np.int32), len(keys),
                    max(acc.values()) if acc else 0, skipped, base_skipped)
