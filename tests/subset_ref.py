"""CPU restatement of the filtered search (csrc/subset.hip, FlatIndexF16.search_filtered): the canonical scores of the ALLOWED
rows, ordered as a search orders them — (score desc, id asc), scores compared by their order-preserving bit pattern, so +0.0
ranks above -0.0; metric "l2": (dist asc, id asc) — and cut at k.  Scores come from the oracle: fp16 rows from
`oracle.cpu_ref.score_rows_f16`, fp32 rows from `oracle.cpu_ref.flat_search_f32` (k = n: every row's canonical score), metric
"l2" from the tests/l2_ref.py restatement.  tests/test_subset_ref_host.py shows this equals "the oracle's full ranking, the
other rows struck out, cut at k"."""
import numpy as np

from tests import l2_ref

_F32 = np.float32


def ordkey(s):
    """rarc_ordkey: the uint32 whose unsigned order is the order of the fp32 scores (a larger key is a better score)."""
    u = np.ascontiguousarray(s, _F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def prepared_queries(oracle, Q, d_pad, normalize):
    Q = np.ascontiguousarray(Q, _F32)
    return oracle.pad_queries(oracle.normalize_L2(Q) if normalize else Q, d_pad)


def allowed_scores(oracle, rows, qp, allowed):
    """Canonical inner products [nq][m] of the prepared queries with the allowed stored rows (uint16 fp16 bits or float32)."""
    allowed = np.ascontiguousarray(allowed, np.int64)
    if allowed.size == 0:
        return np.zeros((qp.shape[0], 0), _F32)
    if rows.dtype == np.uint16:
        return np.stack([oracle.score_rows_f16(rows, qp[i], allowed) for i in range(qp.shape[0])])
    return l2_ref.all_dots(oracle, rows, qp)[:, allowed]


def search(oracle, rows, Q, k, allowed, metric="ip", normalize=False, id_base=0):
    """(D fp32 [nq][k], I int64 [nq][k]) of the filtered search over stored `rows`; padding (-inf, -1), "l2": (+inf, -1)."""
    allowed = np.ascontiguousarray(allowed, np.int64)
    l2 = metric == "l2"
    if l2:
        val = l2_ref.distances(oracle, rows, Q, normalize)[0][:, allowed] if allowed.size else np.zeros((len(Q), 0), _F32)
        key = ordkey(_F32(0.0) - val)                 # (0 - dist: the key the kernels rank by; +0 stays +0)
    else:
        val = allowed_scores(oracle, rows, prepared_queries(oracle, Q, rows.shape[1], normalize), allowed)
        key = ordkey(val)
    nq, kk = val.shape[0], min(int(k), allowed.size)
    D = np.full((nq, k), np.inf if l2 else -np.inf, _F32)
    I = np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        order = np.lexsort((allowed, -key[qi].astype(np.int64)))[:kk]
        D[qi, :kk], I[qi, :kk] = val[qi, order], allowed[order] + id_base
    return D, I


def strike(D_full, I_full, allowed, k, id_base=0, l2=False):
    """The other definition: a full ranking (k = ntotal) with the rows outside `allowed` struck out, cut at k."""
    ok = np.isin(I_full - id_base, allowed) & (I_full >= 0)
    nq = D_full.shape[0]
    D = np.full((nq, k), np.inf if l2 else -np.inf, _F32)
    I = np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        keep = np.flatnonzero(ok[qi])[:k]
        D[qi, :keep.size], I[qi, :keep.size] = D_full[qi, keep], I_full[qi, keep]
    return D, I
