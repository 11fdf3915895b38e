"""The int8 prefilter may only DISCARD rows it can prove irrelevant, so everything hangs on one
inequality:  |canonical(q, d) - approx(q, d)| <= eps8[q]  for every query and every stored row
(csrc/quant.hip, csrc/prep.hip).  Checked here on all pairs of small shards built to stress it:
outlier dimensions, rows and tiles of wildly different magnitude, tiny and huge values, sparse rows,
un-normalised inner-product data.  Also: the bound is not vacuous (eps8 within 3x of the worst error
seen on plain Gaussian data).

Every row format has its own arithmetic behind the same inequality, and each is checked directly:
  fp16 rows   rarc_quant_meta_kernel: tile scale s_t, residual R_t
  fp8 rows    rarc_quant_meta_f8_kernel: s_t, the per-row multiplier mul_r rounded down to fp16, the delta * ||x|| term,
              res = ||x|| for a row that quantises to zeros; approx through rarc_debug_q8_scores_f8
  fp32 rows   the scan reads the fp16 image; its distance rho from the rows (hip/engine.py, qmeta[1]) enters eps8, and the
              canonical score is the one on the fp32 rows
  shadow      the stored int8 image is what the fp16 rows quantise to, byte for byte
The assertion is the inequality, without a tolerance (tests/bound_ref.py); the worst err / eps8 is printed per case."""
import numpy as np
import pytest

from tests import bound_ref as BR

pytestmark = pytest.mark.gpu

STORAGES = ("f16", "f8", "f32")


def _f8_lut():
    from oracle import cpu_ref

    return cpu_ref.f8_decode(np.arange(256, dtype=np.uint8)).astype(np.float64)


def _make(d, metric, storage, shadow=False):
    from rag_arc_amd.hip.engine import FlatIndexF16

    return FlatIndexF16(d, metric=metric, scan="q8", storage=storage, shadow=shadow)


def _check(idx, Q, attained=True):
    """Both forms of the bound for every (query, stored row) of idx; returns the worst err / eps8."""
    import torch

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    n, nq, d_pad = idx.ntotal, Q.shape[0], idx.d_pad
    with idx._lock:
        idx._workspace()
        q = torch.as_tensor(Q, dtype=torch.float32).cuda().contiguous()
        idx._prep(q)
        out = torch.empty((nq, n), dtype=torch.float32, device="cuda")
        qblock = idx._qbuf["qblock"]
        if idx.storage == "f8":
            B.check(lib.rarc_debug_q8_scores_f8(idx._rows.data_ptr(), n, d_pad, idx._qmeta.data_ptr(), qblock.data_ptr(), nq,
                                                out.data_ptr(), 0))
            lut = torch.from_numpy(_f8_lut()).cuda()
            rows = lut[idx.rows.long()] * idx.row_scales.double()[:, None]       # scale * decode(byte): exact in float64
        else:
            scanned = idx._image16 if idx.storage == "f32" else idx._rows          # fp32 rows: the scan reads their fp16 image
            B.check(lib.rarc_debug_q8_scores(scanned.data_ptr(), n, d_pad, idx._qmeta.data_ptr(), qblock.data_ptr(), nq,
                                             out.data_ptr(), 0))
            rows = idx.rows.double()                                               # stored fp16 / fp32 rows, exact in float64
        off = BR.qblock_offsets(d_pad)
        q32 = qblock[: off["q16"]].view(torch.float32).view(BR.MAX_QUERIES, d_pad)[:nq].double()
        exact = q32 @ rows.T                                       # float64: within 1e-12 of the real dot product
        errs = (exact - out.double()).abs().cpu().numpy()
        qb = qblock.cpu().numpy()
        qmeta = idx._qmeta.cpu().numpy()
    eps8, hq = BR.qblock_part(qb, d_pad, "eps8", nq), BR.qblock_part(qb, d_pad, "hq", nq)
    _, rt, _ = BR.tile_meta(qmeta, n, idx.storage)
    ratio = BR.check_bound(errs, eps8, hq, float(qmeta[0]), rt, attained=attained)
    assert (qmeta[1] > 0) == (idx.storage == "f32"), "rho goes with fp32 rows, and only with them"
    return ratio


def _worst_ratio(X, Q, metric, storage="f16"):
    idx = _make(X.shape[1], metric, storage)
    idx.add(X)
    return _check(idx, Q)


def test_bound_holds_and_is_not_vacuous_on_gaussian_data():
    rng = np.random.default_rng(0)
    X = rng.standard_normal((6000, 768)).astype(np.float32)
    Q = rng.standard_normal((64, 768)).astype(np.float32)
    r = _worst_ratio(X, Q, "cosine")
    print(f"err/eps8 f16 gaussian_768: {r:.4f}")
    assert r > 0.02      # Cauchy-Schwarz is ~27x loose on random directions at d=768; far from vacuous


CASES = ["outlier_dims", "row_magnitudes", "tile_magnitudes", "sparse", "tiny_huge", "aligned"]
NEW_CASES = ["norm_spread_in_tile", "one_hot", "tiny_elements", "image_of_zeros", "half_ulp_off_the_image", "zero_rows_zero_query",
             "query_scales", "tiny_queries", "subnormal_queries"]


def _case_data(case, n=4000, d=384, nq=32):
    rng = np.random.default_rng(sum(map(ord, case)))
    X = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    metric = "cosine"
    if case == "outlier_dims":                      # a few dimensions 50x the rest, as in real encoders
        X[:, [3, 77, 200]] *= 50.0
        Q[:, [3, 77, 200]] *= 30.0
    elif case == "row_magnitudes":                  # inner product, row norms over 6 decades
        X *= np.exp(rng.uniform(-7, 7, (n, 1))).astype(np.float32)
        metric = "ip"
    elif case == "tile_magnitudes":                 # whole 32-row tiles tiny or huge
        X *= np.repeat(np.exp(rng.uniform(-6, 6, (n // 32, 1))), 32, axis=0).astype(np.float32)
        metric = "ip"
    elif case == "sparse":                          # 95 % zeros
        X *= (rng.random((n, d)) < 0.05)
        Q *= (rng.random((nq, d)) < 0.2)
    elif case == "tiny_huge":                       # fp16 subnormals next to values near the fp16 maximum
        X[::2] *= 1e-6
        X[1::2] *= 6000.0
        metric = "ip"
    elif case == "aligned":                         # queries parallel to rows: errors add up coherently
        Q = X[:nq].copy() + 0.01 * rng.standard_normal((nq, d)).astype(np.float32)
    elif case == "norm_spread_in_tile":
        # every 32-row tile holds norms from 2^-12 to 2^12: next to the tile's largest row the smallest one's fp8 multiplier
        # mul_r = rowscale * s_t (~ 0.28 * 2^-24) underflows fp16 — the row quantises to zeros, res = ||x|| — and its
        # neighbours' multipliers are fp16 subnormals with few bits (delta far from 0)
        e = np.stack([rng.permutation(np.linspace(-12.0, 12.0, 32)) for _ in range(n // 32)]).reshape(-1, 1)
        X *= np.exp2(e).astype(np.float32)
        metric = "ip"
    elif case == "one_hot":
        # one element carries the whole norm of its row: max|x| * s_t and max|val| * mul_r sit AT 127, where the scale's
        # rounding decides between 127 and 128 (the correction loops behind half_round_down)
        X = np.zeros((n, d), np.float32)
        X[np.arange(n), rng.integers(0, d, n)] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
        metric = "ip"
    elif case == "tiny_elements":
        # elements below 2^-14 (fp16 subnormals) and below 2^-25 (an fp16 image of zeros): for fp32 rows only the ABSOLUTE
        # term of rho covers the distance between the rows and what the scan reads
        X[::2] *= 2.0 ** -16
        X[1::2] *= 2.0 ** -28
        metric = "ip"
    elif case == "image_of_zeros":
        # EVERY element below 2^-25: the fp16 image of an fp32 row is all zeros, approx = 0 and R = 0 — queries parallel to
        # the rows, so the whole score is error, and of the bound only rho's absolute term 2^-25 * sqrt(d_pad) is left
        X *= 2.0 ** -28
        Q = (X[:nq] * 2.0 ** 28).astype(np.float32)
        metric = "ip"
    elif case == "half_ulp_off_the_image":
        # elements +-a, a the largest fp32 that still rounds to the fp16 1.0: the image is off by 2^-11 relative, its int8
        # image is exact (+-127: R = 0) and so is the query's — of the bound only rho's relative term covers q.(d32 - d16)
        a = np.nextafter(np.float32(1.0 + 2.0 ** -11), np.float32(0.0))
        sign = np.where(X >= 0, np.float32(1.0), np.float32(-1.0))
        X, Q, metric = sign * a, sign[:nq].copy(), "ip"
    elif case == "zero_rows_zero_query":
        X[5] = 0.0
        X[64:96] = 0.0                              # a whole tile of zero rows
        X[n - 1] = 0.0
        Q[0] = 0.0
    elif case == "query_scales":
        Q[::2] *= 1e4
        Q[1::2] *= 1e-6
        metric = "ip"
    elif case == "tiny_queries":
        # max|q| just above and just below 127 / FLT_MAX (3.73e-37), where the int8 scale 127 / max|q| is next to FLT_MAX (its
        # inverse a subnormal) or overflows (rarc_query_scale8 then takes 1 and the query quantises to zeros)
        edge = 127.0 / float(np.finfo(np.float32).max)
        to = np.where(np.arange(nq) % 2 == 0, edge * 1.01, edge * 0.99)
        Q = (Q.astype(np.float64) * (to / np.abs(Q).max(axis=1))[:, None]).astype(np.float32)
        assert (np.abs(Q).max(axis=1)[::2] > edge).all() and (np.abs(Q).max(axis=1)[1::2] < edge).all()
        metric = "ip"
    elif case == "subnormal_queries":               # every element an fp32 subnormal (or zero)
        Q = (Q.astype(np.float64) * 1e-42).astype(np.float32)
        assert Q.any() and np.abs(Q).max() < np.finfo(np.float32).tiny
        metric = "ip"
    else:
        raise KeyError(case)
    return X, Q, metric


@pytest.mark.parametrize("case", CASES)
def test_bound_holds_on_adversarial_data(case):
    X, Q, metric = _case_data(case)
    print(f"err/eps8 f16 {case}: {_worst_ratio(X, Q, metric):.4f}")


@pytest.mark.parametrize("case", NEW_CASES)
def test_bound_holds_on_edge_data_f16(case):
    X, Q, metric = _case_data(case)
    print(f"err/eps8 f16 {case}: {_worst_ratio(X, Q, metric):.4f}")


@pytest.mark.parametrize("case", CASES + NEW_CASES)
@pytest.mark.parametrize("storage", ["f8", "f32"])
def test_bound_holds_on_fp8_and_fp32_rows(storage, case):
    """The same data through the other two derivations of the bound.  No floor on err / eps8 here: it is printed."""
    X, Q, metric = _case_data(case)
    print(f"err/eps8 {storage} {case}: {_worst_ratio(X, Q, metric, storage):.4f}")


@pytest.mark.parametrize("d", [1, 100, 300, 1024])
@pytest.mark.parametrize("storage", STORAGES)
def test_bound_at_the_shapes_where_the_paths_differ(storage, d):
    """d: the smallest there is, two off the padding grid (padded columns in play), the narrow path's maximum.  n: a single
    row, either side of one tile, and a ragged last tile.  nq: one query and a full block."""
    rng = np.random.default_rng(1000 * d + len(storage))
    worst = 0.0
    for n in (1, 31, 33, 4000, 4001):
        for nq in (1, 256):
            metric = "ip" if (n + nq) % 2 else "cosine"
            X = rng.standard_normal((n, d)).astype(np.float32)
            if metric == "ip":
                X *= np.exp(rng.uniform(-2, 2, (n, 1))).astype(np.float32)
            Q = rng.standard_normal((nq, d)).astype(np.float32)
            worst = max(worst, _worst_ratio(X, Q, metric, storage))
    print(f"err/eps8 {storage} shapes d={d}: {worst:.4f}")


def _tile_state(idx):
    qm = idx._qmeta.cpu().numpy()
    return float(qm[0]), BR.tile_meta(qm, idx.ntotal, idx.storage)


@pytest.mark.parametrize("state", ["two_adds", "removed_a_third"])
@pytest.mark.parametrize("storage", STORAGES)
def test_bound_across_the_index_lifecycle(storage, state):
    """Tile metadata is recomputed for the tiles a change touches, R is only ever raised.  Rows whose magnitude differs from
    tile to tile: after the change every s_t / R_t must fit the rows that are in the tile NOW."""
    n, d = 4001, 300
    X, Q, metric = _case_data("tile_magnitudes", n=n - 1, d=d)
    X = np.concatenate([X, X[:1] * 3.0])
    idx = _make(d, metric, storage)
    if state == "two_adds":
        idx.add(X[:1009])                      # ends 17 rows into tile 31: the second add recomputes that tile
        R0 = _tile_state(idx)[0]
        idx.add(X[1009:])
    else:
        idx.add(X)
        R0 = _tile_state(idx)[0]
        assert idx.remove_rows(np.arange(1, n, 3)) == len(range(1, n, 3))      # compaction moves rows between tiles
    R1, (s, rt, inv) = _tile_state(idx)
    assert R1 >= R0, "R may only stay or grow"
    assert (s > 0).all() and (inv > 0).all()
    print(f"err/eps8 {storage} {state}: {_check(idx, Q, attained=False):.4f}")


@pytest.mark.parametrize("case", ["gaussian", "tile_magnitudes", "tiny_huge", "one_hot", "zero_rows_zero_query"])
def test_shadow_image_is_the_int8_image_of_the_rows(case):
    """The stored int8 image, every byte of every row: what the fp16 rows quantise to under their tile's scale (restated on
    the host, tests/bound_ref.py), and what the score hook — which quantises the fp16 rows itself, with the scan's own
    routine — must have summed: its scores are reproduced bit for bit from the image.  Then across a second add and a
    removal."""
    import torch

    from rag_arc_amd.hip import binding as B

    n, d = 4001, 256
    X, Q, metric = _case_data("aligned" if case == "gaussian" else case, n=n - 1, d=d)
    X = np.concatenate([X, X[:1] * 3.0])
    idx = _make(d, metric, "f16", shadow=True)
    idx.add(X[:1009])
    idx.add(X[1009:])
    lib = B.load_library()
    for step in ("added", "removed"):
        if step == "removed":
            idx.remove_rows(np.arange(1, n, 3))
        m = idx.ntotal
        qm = idx._qmeta.cpu().numpy()
        s, _, inv = BR.tile_meta(qm, m, "f16")
        image = idx._shadow[:m].cpu().numpy()
        want = BR.int8_image_f16(idx.rows.cpu().numpy(), s)
        assert np.array_equal(image, want), f"{step}: {int((image != want).sum())} bytes of the image differ"
        _check(idx, Q, attained=False)              # (leaves the query block prepared)
        nq = Q.shape[0]
        out = torch.empty((nq, m), dtype=torch.float32, device="cuda")
        B.check(lib.rarc_debug_q8_scores(idx._rows.data_ptr(), m, idx.d_pad, idx._qmeta.data_ptr(),
                                         idx._qbuf["qblock"].data_ptr(), nq, out.data_ptr(), 0))
        qb = idx._qbuf["qblock"].cpu().numpy()
        q8 = BR.qblock_part(qb, idx.d_pad, "q8", nq).astype(np.float64)
        qinv = BR.qblock_part(qb, idx.d_pad, "qinv", nq)
        acc = (q8 @ image.astype(np.float64).T).astype(np.float32)                 # integers below 2^24: exact
        tinv = np.repeat(inv.astype(np.float32), 32)[:m]
        again = acc * (qinv[:, None] * tinv[None, :])
        assert np.array_equal(again.view(np.uint32), out.cpu().numpy().view(np.uint32)), f"{step}: scores differ from the image's"
