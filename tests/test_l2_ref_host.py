"""The CPU restatement of metric "l2" (tests/l2_ref.py) against float64 sum((q - x)^2) over the stored rows — no GPU.

Bound.  A canonical dot is d_pad / 8 FMAs per chain plus three additions of the tree: |dot - exact| <= (d_pad/8 + 3) u S
to first order, u = 2^-24, S the sum of the |products| (S = qn, xn for the norms, S = sum |q_i x_i| =: A for ip).  Then
t = fl(qn + xn) adds u (qn + xn) and dist = fl(t - 2 ip) adds u |dist| <= u (qn + xn + 2 |ip|); the clamp at 0 only moves a
value towards the (non-negative) truth.  Together
    |dist - sum (q - x)^2| <= (qn + xn + 2 A) (d_pad/8 + 5) 2^-24           (A >= |ip|, 2 A <= qn + xn)
which is the derived form of the issue's (qn + xn + 2 |ip|) (d/8 + 4) 2^-24: A replaces |ip| because the chains' roundings
scale with the magnitudes of the products, not with their (cancelling) sum, and the two final roundings count one each.
(1.001 covers the second-order terms: d_pad/8 * u <= 3e-5.)"""
import numpy as np
import pytest

from tests import l2_ref

DIMS = [64, 384, 768, 1536]


def _data(d, spread, seed):
    rng = np.random.default_rng(seed)
    n, nq = 300, 6
    X = rng.standard_normal((n, d)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    if spread:        # norms over two decades, 0.1 .. 10
        X *= (10.0 ** rng.uniform(-1, 1, (n, 1))).astype(np.float32)
        Q *= (10.0 ** rng.uniform(-1, 1, (nq, 1))).astype(np.float32)
    X[7] = X[3]                                   # a duplicate row
    Q[0] = X[11].astype(np.float16).astype(np.float32)      # a query that IS a stored fp16 row
    return X, Q


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic, the fp32 ties a float64 sum cannot see included."""
    from fractions import Fraction

    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    # planted: a*b = 2^-24 - 2^-70, so the float64 sum with c lands exactly ON an fp32 midpoint and only the TwoSum residual
    # says which side the true sum lies on (ties-to-even alone would round 1 + 2^-23 + 2^-24 - 2^-70 up)
    a[:2] = np.float32(2.0 ** -12 * (1 + 2.0 ** -23))
    b[:2] = np.float32(2.0 ** -12 * (1 - 2.0 ** -23))
    c[:2] = np.array([1.0 + 2.0 ** -23, 1.0], np.float32)
    a[2:6], b[2:6] = np.float32(1.0), np.float32(2.0 ** -24)           # c + 2^-24: exact ties (ties to even)
    c[2:6] = np.array([1.0, 1.0 + 2.0 ** -23, -1.0, 2.0], np.float32)
    got = l2_ref.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))             # float(Fraction) rounds correctly to float64; refine to fp32 by comparison
        cands = {np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))}
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert np.float32(got[i]).view(np.uint32) == np.float32(best).view(np.uint32), (i, a[i], b[i], c[i])


@pytest.mark.parametrize("d", DIMS)
def test_canon_dot_is_the_oracles(oracle, d):
    """canon_dot (numpy, exact FMAs) == the oracle's canonical scores, bit for bit: fp32 rows and fp16 rows."""
    X, Q = _data(d, True, d)
    rows32 = l2_ref.stored_rows(oracle, X, "f32")
    rows16 = l2_ref.stored_rows(oracle, X, "f16")
    qp = oracle.pad_queries(Q, rows32.shape[1])
    for rows, as32 in ((rows32, rows32), (rows16, rows16.view(np.float16).astype(np.float32))):
        ref = l2_ref.all_dots(oracle, rows, qp)
        got = l2_ref.canon_dot(qp[:, None, :], as32[None, :, :])
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    x16 = rows16.view(np.float16).astype(np.float32)
    assert np.array_equal(l2_ref.sqnorms_f16(rows16).view(np.uint32), l2_ref.canon_dot(x16, x16).view(np.uint32))


@pytest.mark.parametrize("storage", ["f16", "f32"])
@pytest.mark.parametrize("spread", [False, True], ids=["unit", "spread"])
@pytest.mark.parametrize("d", DIMS)
def test_restatement_against_float64(oracle, d, spread, storage):
    X, Q = _data(d, spread, 100 + d)
    rows = l2_ref.stored_rows(oracle, X, storage)
    d_pad = rows.shape[1]
    dist, xn, qn = l2_ref.distances(oracle, rows, Q)
    x64 = (rows.view(np.float16) if storage == "f16" else rows).astype(np.float64)
    q64 = oracle.pad_queries(Q, d_pad).astype(np.float64)
    exact = ((q64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2)
    A = np.abs(q64[:, None, :] * x64[None, :, :]).sum(axis=2)
    bound = (qn.astype(np.float64)[:, None] + xn.astype(np.float64)[None, :] + 2.0 * A) * (d_pad / 8 + 5) * 2.0 ** -24 * 1.001
    err = np.abs(dist.astype(np.float64) - exact)
    print(f"d={d} spread={spread} {storage}: max |err| / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    assert (dist >= 0).all()
    if storage == "f16":
        assert dist[0, 11] == 0.0 and not np.signbit(dist[0, 11])          # the query bit-equal to a stored row
    # order: wherever float64 separates two rows by more than both bounds, the restatement orders them the same way
    D, I = l2_ref.search(oracle, X, Q, X.shape[0], storage, rows=rows)
    for qi in range(Q.shape[0]):
        assert np.array_equal(D[qi], dist[qi, I[qi]]) and (np.diff(D[qi]) >= 0).all()
        tied = np.diff(D[qi]) == 0
        assert (np.diff(I[qi])[tied] > 0).all()                             # ties by id ascending
        rank = np.empty(X.shape[0], np.int64)
        rank[I[qi]] = np.arange(X.shape[0])
        gap = exact[qi][None, :] - exact[qi][:, None]                       # gap[i][j] = exact_j - exact_i
        clear = gap > 2.0 * np.maximum(bound[qi][None, :], bound[qi][:, None])
        ii, jj = np.nonzero(clear)
        assert (rank[ii] < rank[jj]).all()
    assert (rank[3] + 1 == rank[7])                                         # the duplicate pair: adjacent, lower id first


def test_normalised_rows_and_queries(oracle):
    """normalize=True: both sides normalised as for cosine, then the same definition; distances within 2 - 2 cos."""
    X, Q = _data(384, True, 9)
    rows = l2_ref.stored_rows(oracle, X, "f16", normalize=True)
    dist, xn, qn = l2_ref.distances(oracle, rows, Q, normalize=True)
    assert np.abs(xn - 1).max() < 2e-3 and np.abs(qn - 1).max() < 1e-5
    cos = l2_ref.all_dots(oracle, rows, oracle.pad_queries(oracle.normalize_L2(Q), rows.shape[1]))
    assert np.abs(dist - (2 - 2 * cos)).max() < 5e-3
