"""The wide path (csrc/wide.hip) is exact only because eps[q] — and eps_k, delta under metric "l2" — from wide_eps_kernel
bound the error of the approximate scores, and thr is only ever rounded down.  The inequalities are asserted here directly,
in float64 and without a tolerance (the kernel rounds its bound outward), from what a search leaves in its workspace
(rarc_debug_wide_bounds: eps, the final thr, epsd, qn) and the query block (q32, q16):

  eps        eps[q] >= |dot64(q16, x16) - canonical(q32, x)| for every stored row: q16 the fp16 query as rarc_prep_queries
             rounds it, x16 the fp16 row (the fp16 image of an fp32 row), canonical the oracle's score.  The real approximate
             score differs from dot64 by accumulation and fp16-store error, which eps has to cover too: an eps below this
             value is wrong, one above it is not thereby right.
  thr        cosine / ip: thr[q] <= L_q - eps[q], L_q the oracle's k-th best canonical score (thr = a_k - 2 eps, L >= a_k - eps)
             l2: thr[q] <= min(kappa_k, qn / 2) - epsd[q], kappa_k the k-th largest ip - xn / 2 (float64, canonical ip, stored
             xn); qn is l2_ref's canonical |q|^2 bit for bit; and epsd[q] - eps[q], the kernel's delta, covers
             |dist - max(0, qn - 2 kappa)| of every row (epsd alone would hide a missing delta behind the slack of eps_k)
  padding    queries beyond nq keep thr = +inf

The data presses on one term of wide_eps_kernel each (see _case); every premise is checked on the CPU from the oracle before
the GPU is touched.  Metric "ip" with the power-of-two query scaling engaged is compared in the SCALED domain: q32, q16, eps
and thr all belong to the scaled queries the library was given.  max_r |dot64 - canonical| / eps[q] is printed per case — a
measurement (DESIGN.md has the observed range), not asserted from above."""
import numpy as np
import pytest

from tests import bound_ref as BR
from tests import l2_ref
from tests import wide_ref as WR

pytestmark = pytest.mark.gpu

FIRST = 16384


def _f16(a):
    return np.asarray(a, np.float32).astype(np.float16)


def _midpoints(rng, shape, lo=-3, hi=3):
    """fp32 values exactly between two neighbouring fp16 values just above a power of two: (1 + (2m + 1) 2^-11) 2^e, m < 8."""
    m = rng.integers(0, 8, shape)
    v = (1.0 + (2 * m + 1) * 2.0 ** -11) * np.exp2(rng.integers(lo, hi + 1, shape)) * rng.choice([-1.0, 1.0], shape)
    v = v.astype(np.float32)
    assert (np.abs(v.astype(np.float64) - _f16(v).astype(np.float64)) == np.exp2(np.floor(np.log2(np.abs(v))) - 11)).all()
    return v


def _prepared(oracle, Q, metric):
    """The query as rarc_prep_queries leaves it (before any power-of-two scaling): normalised for cosine."""
    return oracle.normalize_L2(Q) if metric == "cosine" else np.ascontiguousarray(Q, np.float32)


def _aligned_rows(oracle, Q, metric, norm):
    """Per query the row of length `norm` along its rounding error q32 - q16."""
    q = _prepared(oracle, Q, metric).astype(np.float64)
    dq = q - _f16(q).astype(np.float64)
    return (dq / np.linalg.norm(dq, axis=1, keepdims=True) * norm).astype(np.float32)


def _case(oracle, name):
    """-> dict(metric, storage, X, Q, k, aligned: rows planted along the queries' rounding errors or None)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    c = dict(metric="cosine", storage="f16", k=1025, aligned=None)
    if name.startswith("midpoints_"):
        # query elements on fp16 rounding midpoints — normal ones (queries 0..3) and subnormal ones, (j + 1/2) 2^-24, where
        # the rounding error is a third of the element and more (4..7) — and per query a row of the largest norm along
        # q32 - q16: the sqrt(dn) * mn term, nearly attained.  Under cosine the normalisation moves the elements off the
        # midpoints; the row is aligned with the error that is left.
        c["metric"] = name.split("_")[1]
        d, n = 256, FIRST + 512 + 77
        X = rng.standard_normal((n, d)).astype(np.float32) * np.float32(0.5)
        Q = _midpoints(rng, (8, d))
        Q[4:] = ((rng.integers(0, 4, (4, d)) + 0.5) * 2.0 ** -24 * rng.choice([-1.0, 1.0], (4, d))).astype(np.float32)
        big = 1.0 if c["metric"] == "cosine" else 1.05 * float(np.linalg.norm(X, axis=1).max())
        c["aligned"] = list(range(n - 8, n))                  # in the last chunk
        X[n - 8:] = _aligned_rows(oracle, Q, c["metric"], big)
    elif name == "dominant_4096":
        # cosine, d = 4096, one element carries the norm: after normalisation nearly all of q16 is subnormal or zero
        d, n, c["k"] = 4096, 3000, 10
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = (rng.standard_normal((4, d)) * np.exp2(rng.uniform(-22, -15, (4, d)))).astype(np.float32)
        Q[:, 0] = 1.0
        c["aligned"] = list(range(n - 4, n))
        X[n - 4:] = _aligned_rows(oracle, Q, "cosine", 1.0)
    elif name.startswith("gauss_"):
        # d_pad = 256, 1152 (d = 1088: rows pad to multiples of 128) and 4096: the d_pad * 2^-23 term
        d = int(name.split("_")[1])
        n = FIRST + 300 if d == 256 else 3000
        c["k"] = 1025 if d == 256 else 10
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((8, d)).astype(np.float32)
    elif name in ("tiny_queries", "subnormal_queries"):
        # metric "ip" at the small end of the fp32 range, the shape of gauss_256: max|q| just above / just below 127 / FLT_MAX
        # (where the query block's int8 scale is next to FLT_MAX, or overflows and falls back to 1), and queries whose every
        # element is an fp32 subnormal.  q16 is all zeros: the whole canonical score is error, and eps has to cover it.
        c["metric"] = "ip"
        d, n = 256, FIRST + 300
        X = rng.standard_normal((n, d)).astype(np.float32)
        Q = rng.standard_normal((8, d))
        if name == "tiny_queries":
            edge = 127.0 / float(np.finfo(np.float32).max)
            Q = (Q * (np.where(np.arange(8) % 2 == 0, edge * 1.01, edge * 0.99) / np.abs(Q).max(axis=1))[:, None]).astype(np.float32)
            assert (np.abs(Q).max(axis=1)[::2] > edge).all() and (np.abs(Q).max(axis=1)[1::2] < edge).all()
        else:
            Q = (Q * 1e-42).astype(np.float32)
            assert Q.any() and np.abs(Q).max() < np.finfo(np.float32).tiny
    elif name == "f32_rows_off_their_image":
        # fp32 storage, every row element on an fp16 midpoint: ||row - image|| is the whole 2^-11 ||row|| that rho allows, and
        # the queries run along row - image of the heaviest rows
        c.update(metric="ip", storage="f32")
        d, n = 256, FIRST + 512 + 5
        X = _midpoints(rng, (n, d), lo=-2, hi=0)
        heavy = np.argsort(-np.linalg.norm(X.astype(np.float64), axis=1))[:8]
        off = X[heavy].astype(np.float64) - _f16(X[heavy]).astype(np.float64)
        Q = _f16(off / np.abs(off).max(axis=1, keepdims=True)).astype(np.float32)         # exact in fp16: dn = 0
    elif name == "ip_scaled_queries":
        # |q| * max |row| ~ 1900 * 26 >= 2^15: the engine hands the queries over scaled by a power of two
        c["metric"] = "ip"
        d, n = 256, FIRST + 256 + 3
        X = rng.standard_normal((n, d)).astype(np.float32) * np.float32(1.5)
        Q = rng.standard_normal((8, d)).astype(np.float32) * np.float32(120.0)
    elif name.startswith("l2_spread_"):
        # norms over two decades, query 0 a stored row (distance 0: the clamp), query 1 a tiny one (qn / 2 under every kappa
        # but its own neighbourhood's: the qn / 2 branch), query 2 a heavy one
        c.update(metric="l2", storage=name.split("_")[2], k=10)
        d, n = (64, FIRST + 512 + 77) if c["storage"] == "f16" else (256, 5000)
        X = rng.standard_normal((n, d)).astype(np.float32)
        X *= (10.0 ** rng.uniform(-1, 1, (n, 1)) / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
        Q = rng.standard_normal((6, d)).astype(np.float32)
        Q *= (10.0 ** rng.uniform(-1, 1, (6, 1)) / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
        X[n - 5] = _f16(X[n - 5]).astype(np.float32)
        Q[0] = X[n - 5]
        Q[1] *= np.float32(0.05 / np.linalg.norm(Q[1]))
        Q[2] *= np.float32(10.0 / np.linalg.norm(Q[2]))
        X[7] = Q[1]
        X[n - 9] = Q[1]
        for r in list(range(100, 106)) + [n - 5 - 37 * i for i in range(1, 12)]:       # 18 copies of query 0's row, k = 10: the k-th
            X[r] = X[n - 5]                                                          # smallest distance is 0, the qn / 2 branch
    else:
        raise KeyError(name)
    c.update(X=X, Q=Q)
    return c


CASES = ["midpoints_ip", "midpoints_cosine", "dominant_4096", "gauss_256", "gauss_1088", "gauss_4096", "f32_rows_off_their_image",
         "ip_scaled_queries", "l2_spread_f16", "l2_spread_f32", "tiny_queries", "subnormal_queries"]
LATER_CHUNKS = {"midpoints_ip": "fused128", "midpoints_cosine": "fused128", "gauss_256": "fused128",
                "f32_rows_off_their_image": "fused128", "ip_scaled_queries": "fused128", "l2_spread_f16": "stored",
                "tiny_queries": "fused128", "subnormal_queries": "fused128"}


def _search_and_bounds(idx, Q, k):
    """One batch through _search_wide_chunk, then the hook on the workspace it used.  -> (D, I, bounds [4][256], q32, q16)"""
    import torch

    from rag_arc_amd.hip import binding as B

    nq = Q.shape[0]
    with idx._lock, torch.cuda.device(idx.device):
        q = torch.as_tensor(Q, dtype=torch.float32).to(idx.device).contiguous()
        ids = torch.empty((nq, k), dtype=torch.int64, device=idx.device)
        sc = torch.empty((nq, k), dtype=torch.float32, device=idx.device)
        idx._search_wide_chunk(q, k, ids, sc)
        out = torch.empty((4, BR.MAX_QUERIES), dtype=torch.float32, device=idx.device)
        B.check(idx.lib.rarc_debug_wide_bounds(idx._wide_ws.data_ptr(), idx._wide_ws.numel(), idx.d_pad, idx.last_wide_cap,
                                               out.data_ptr(), idx._stream()), "rarc_debug_wide_bounds")
        torch.cuda.synchronize()
        qb = idx._qbuf["qblock"].cpu().numpy()
        return (sc.cpu().numpy(), ids.cpu().numpy(), out.cpu().numpy(), BR.qblock_part(qb, idx.d_pad, "q32", nq).copy(),
                BR.qblock_part(qb, idx.d_pad, "q16", nq).copy())


@pytest.mark.parametrize("name", CASES)
def test_wide_bounds(oracle, name):
    from rag_arc_amd.hip.engine import FlatIndexF16

    c = _case(oracle, name)
    metric, storage, X, Q, k = c["metric"], c["storage"], c["X"], c["Q"], c["k"]
    n, d = X.shape
    nq, d_pad = Q.shape[0], oracle.padded_dim(d)
    normalize = metric == "cosine"
    # ---- the premises, from the oracle alone
    later = [p.form for p in WR.plan(n, k, d_pad)[1:]]
    assert later == ([LATER_CHUNKS[name]] if name in LATER_CHUNKS else []), (name, later)
    rows = l2_ref.stored_rows(oracle, X, storage, normalize)
    x16 = WR.image16(rows)
    assert np.isfinite(x16.astype(np.float32)).all()
    norms = np.linalg.norm((rows.view(np.float16) if storage == "f16" else rows).astype(np.float64), axis=1)
    qp = oracle.pad_queries(_prepared(oracle, Q, metric), d_pad)
    unscale = 1.0
    if metric == "ip":
        bound = float(np.linalg.norm(qp.astype(np.float64), axis=1).max()) * float(norms.max())
        if bound * 1.01 >= 32768.0:          # the engine's power-of-two scaling (hip/engine.py: _search_wide_chunk), restated
            unscale = 2.0 ** (int(np.ceil(np.log2(bound * 1.01 / 32768.0))) + 1)
            qp = (qp * np.float32(1.0 / unscale)).astype(np.float32)
    assert (unscale != 1.0) == (name == "ip_scaled_queries")
    d64 = WR.dot64(_f16(qp), x16)
    assert np.abs(d64[:, :WR.plan(n, k, d_pad)[0].rows]).max() < 65504.0 * 0.99, "the first chunk's fp16 scores are finite"
    canon = l2_ref.all_dots(oracle, rows, qp).astype(np.float64)
    err = np.abs(d64 - canon)
    if c["aligned"] is not None:            # the planted row nearly attains ||q32 - q16|| * (largest norm)
        dq = np.linalg.norm(qp.astype(np.float64) - _f16(qp).astype(np.float64), axis=1)
        for j, r in enumerate(c["aligned"]):
            assert norms[r] >= 0.94 * norms.max() and err[j, r] >= 0.9 * dq[j] * norms[r] > 0, (name, j, err[j, r], dq[j] * norms[r])
        if name == "dominant_4096":
            assert (np.abs(_f16(qp[:, 1:d]).astype(np.float32)) < 2.0 ** -14).mean() > 0.99, "q16 is subnormal but for one element"
    if name == "f32_rows_off_their_image":  # every row sits 2^-11 (relative, elementwise) off its image: what rho has to carry
        off = np.linalg.norm(rows.astype(np.float64) - x16.astype(np.float64), axis=1)
        assert (off >= 0.99 * 2.0 ** -11 * np.linalg.norm(x16.astype(np.float64), axis=1)).all()
        assert (qp == _f16(qp).astype(np.float32)).all() and err.max(axis=1).min() > 0.5 * off.max() * np.linalg.norm(qp[0])
    # ---- the search and what it left behind
    idx = FlatIndexF16(d, metric=metric, storage=storage)
    idx.add(X)
    D, I, bounds, q32, q16 = _search_and_bounds(idx, Q, k)
    eps, thr, epsd, qn = (bounds[i].astype(np.float64) for i in range(4))
    stored = idx.rows.cpu().numpy()
    assert np.array_equal(stored.view(rows.dtype) if storage == "f16" else stored, rows), "the stored rows are the oracle's"
    assert np.array_equal(q32.view(np.uint32), qp.view(np.uint32)), "q32 is the prepared (and scaled) query"
    assert np.array_equal(q16.view(np.uint16), _f16(qp).view(np.uint16)), "q16 is q32 rounded to nearest even"
    assert np.isposinf(thr[nq:]).all(), "padding queries keep thr = +inf"
    assert np.isfinite(eps[:nq]).all() and (eps[:nq] > 0).all() and np.isfinite(thr[:nq]).all()
    ratio = err.max(axis=1) / eps[:nq]
    print(f"wide err/eps {name}: {ratio.min():.4f} .. {ratio.max():.4f}")
    assert (err <= eps[:nq, None]).all(), f"eps too small: worst err/eps = {ratio.max():.4f} (query {int(ratio.argmax())})"
    if metric == "l2":
        dist, xn, qn_ref = l2_ref.distances(oracle, rows, Q)
        assert np.array_equal(bounds[3, :nq].view(np.uint32), qn_ref.view(np.uint32)), "qn is the canonical |q|^2"
        assert np.array_equal(idx.row_sqnorms.cpu().numpy().view(np.uint32), xn.view(np.uint32))
        kappa = WR.l2_kappa(canon, xn)
        limit = np.minimum(WR.kth_largest(kappa, k), 0.5 * qn[:nq]) - epsd[:nq]
        assert (thr[:nq] <= limit).all(), f"thr above min(kappa_k, qn/2) - epsd by {(thr[:nq] - limit).max():.3e}"
        derr = WR.l2_dist_error(dist, qn_ref, kappa)
        delta = epsd[:nq] - eps[:nq]
        print(f"wide dist-err/delta {name}: {(derr / delta).min():.4f} .. {(derr / delta).max():.4f}")
        assert derr.max() > 0 and (delta >= derr).all(), f"epsd - eps does not cover the rounding of dist: {delta} < {derr}"
        assert np.sort(dist[0])[k - 1] == 0.0, "query 0: k rows at distance 0 (the clamp, and the qn / 2 branch of thr)"
        ref_D, ref_I = l2_ref.search(oracle, X, Q, k, storage, rows=rows)
    else:
        L = WR.kth_largest(canon, k)
        assert (thr[:nq] <= L - eps[:nq]).all(), f"thr above L - eps by {(thr[:nq] - (L - eps[:nq])).max():.3e}"
        order = np.lexsort((np.broadcast_to(np.arange(n), canon.shape), -canon), axis=1)[:, :k]
        ref_I, ref_D = order, (np.take_along_axis(canon, order, axis=1) * unscale).astype(np.float32)
    assert np.array_equal(I, ref_I) and np.array_equal(D.view(np.uint32), ref_D.view(np.uint32)), "and the answer is the oracle's"


def test_the_hook_validates_its_arguments():
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    assert lib.rarc_debug_wide_bounds(None, 1 << 30, 256, 16640, None, None) == -1
