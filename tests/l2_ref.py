"""CPU restatement of metric "l2" (csrc/wide.hip): with dot() the project's canonical fp32 inner product
(eight FMA chains over elements 8m + j, then the fixed tree),

    qn = dot(q, q)    xn = dot(x, x)    ip = dot(q, x)    dist = max(0, (qn + xn) - 2 ip)       every operation fp32

ordered by (dist ascending, id ascending); x is the STORED row (fp16-rounded for storage "f16", the fp32 row for "f32"), and
with normalize=True rows and queries are normalised first exactly as for cosine.

ip comes from the oracle's own searches with k = n (canonical scores of every row).  qn and xn restate the chains in numpy:
for fp16-representable values a product is exact in fp32, so fma(x, x, a) is one fp32 addition; for fp32 values fma32() below
rounds the exact a*b + c once (float64 product — 48 bits, exact — then a TwoSum decides the rare fp32 tie the float64 sum
cannot see).  canon_dot() is held to the oracle bit for bit in tests/test_l2_ref_host.py.
"""
import numpy as np

_F32, _F64 = np.float32, np.float64


def fma32(a, b, c):
    """fp32 fused multiply-add, one rounding: float32(a*b + c) for float32 arrays (no overflow / subnormal handling)."""
    p = np.asarray(a, _F32).astype(_F64) * np.asarray(b, _F32).astype(_F64)        # exact: 24 + 24 bits
    c64 = np.asarray(c, _F32).astype(_F64)
    s = p + c64
    bb = s - p
    err = (p - (s - bb)) + (c64 - bb)                                               # TwoSum: p + c64 = s + err exactly
    f = s.astype(_F32)
    d = s - f.astype(_F64)                                                          # exact
    maybe = (d != 0) & (err != 0)
    if maybe.any():
        other = np.nextafter(f, np.where(d > 0, _F32(np.inf), _F32(-np.inf)).astype(_F32))
        tie = maybe & ((other.astype(_F64) - s) == d)                               # s sits exactly between f and other
        away = tie & (np.sign(err) == np.sign(d))                                   # the true sum lies on other's side
        f = np.where(away, other, f)
    return f.astype(_F32)


def _tree(acc):
    return ((acc[..., 0] + acc[..., 4]) + (acc[..., 2] + acc[..., 6])) + ((acc[..., 1] + acc[..., 5]) + (acc[..., 3] + acc[..., 7]))


def canon_dot(a, b):
    """Canonical fp32 dot of the rows of a with the rows of b (float32 [..][d_pad], d_pad a multiple of 8), exact FMAs."""
    a, b = np.asarray(a, _F32), np.asarray(b, _F32)
    acc = np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]) + (8,), _F32)
    for m in range(a.shape[-1] // 8):
        acc = fma32(a[..., 8 * m: 8 * m + 8], b[..., 8 * m: 8 * m + 8], acc)
    return _tree(acc)


def sqnorms_f16(rows_u16):
    """Canonical dot(x, x) of fp16 rows (uint16 bit patterns [n][d_pad]): the squares are exact in fp32."""
    n, d_pad = rows_u16.shape
    acc = np.zeros((n, 8), _F32)
    for m in range(d_pad // 8):
        x = rows_u16[:, 8 * m: 8 * m + 8].view(np.float16).astype(_F32)
        acc = acc + x * x
    return _tree(acc)


def stored_rows(oracle, X, storage="f16", normalize=False):
    """The rows as the index stores them: uint16 bit patterns [n][d_pad] (f16) or float32 [n][d_pad] (f32)."""
    X = np.ascontiguousarray(X, _F32)
    return oracle.ingest_f32(X, normalize=normalize)[0] if storage == "f32" else oracle.ingest_f16(X, normalize=normalize)[0]


def all_dots(oracle, rows, qp):
    """ip[nq][n]: the oracle's canonical score of every stored row for every query."""
    n = rows.shape[0]
    if rows.dtype == np.uint16:
        ids, sc, _ = oracle.flat_search_f16(rows, qp, n)
    else:
        ids, sc = oracle.flat_search_f32(rows, qp, n)[:2]
    out = np.empty_like(sc)
    np.put_along_axis(out, ids, sc, axis=1)
    return out


def distances(oracle, rows, Q, normalize=False):
    """(dist fp32 [nq][n], xn fp32 [n], qn fp32 [nq]) of the definition above for stored rows and raw queries Q."""
    d_pad = rows.shape[1]
    qp = oracle.pad_queries(oracle.normalize_L2(Q) if normalize else np.ascontiguousarray(Q, _F32), d_pad)
    qn = canon_dot(qp, qp)
    xn = sqnorms_f16(rows) if rows.dtype == np.uint16 else canon_dot(rows, rows)
    ip = all_dots(oracle, rows, qp)
    t = (qn[:, None] + xn[None, :]).astype(_F32)
    d = (t - _F32(2.0) * ip).astype(_F32)             # 2 ip is exact: one rounding
    return np.where(d > 0, d, _F32(0.0)).astype(_F32), xn, qn


def search(oracle, X, Q, k, storage="f16", normalize=False, id_base=0, rows=None):
    """(D fp32 [nq][k] ascending, I int64 [nq][k]): the exact L2 top-k; (+inf, -1) beyond the stored rows."""
    rows = stored_rows(oracle, X, storage, normalize) if rows is None else rows
    dist, _, _ = distances(oracle, rows, Q, normalize)
    nq, n = dist.shape
    kk = min(k, n)
    D = np.full((nq, k), np.inf, _F32)
    I = np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        order = np.lexsort((np.arange(n), dist[qi]))[:kk]
        D[qi, :kk], I[qi, :kk] = dist[qi, order], order + id_base
    return D, I


def ip_topk(oracle, X, Q, k, storage="f16", normalize=False):
    """ids of the inner-product top-k of the same stored rows (what the L2 answer must differ from on spread norms)."""
    rows = stored_rows(oracle, X, storage, normalize)
    qp = oracle.normalize_L2(Q) if normalize else np.ascontiguousarray(Q, _F32)
    if storage == "f32":
        return oracle.flat_search_f32(rows, qp, k)[0]
    return oracle.flat_search_f16(rows, qp, k)[0]
