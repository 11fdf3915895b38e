"""Layout arithmetic and the two inequalities behind the int8 prefilter, restated on the host (numpy only) for the tests
that check them on the device (tests/test_gpu_q8_bound.py) and held to hand-made examples in tests/test_bound_ref_host.py.

Query block (csrc/rarc_common.h, rarc_qb_carve), bytes from its base, nqd = 256 * d_pad:
    q32 f32 [256][d_pad] @ 0 | q16 f16 @ 4 nqd | q8 i8 @ 6 nqd | eps16 f32 [256] @ 7 nqd | eps8 @ +1024 | qinv @ +2048
    | hq @ +3072 | floor @ +4096
Quantisation metadata (floats): [0] R, [1] rho, [2..3] reserved, then per 32-row tile t at 4 + stride * t:
    [0] one word: low half = fp16 bits of the scale s_t, high half = fp16 bits of R_t rounded up;  [1] 1 / s_t;
    fp8 rows only (stride 34 instead of 2): [2 + r] the fp16-representable multiplier of row r of the tile.

The bound, for every query q and stored row r of tile t:
    global    |canonical(q, r) - approx(q, r)| <= eps8[q]
    per tile  |canonical(q, r) - approx(q, r)| <= eps8[q] - hq[q] * max(0, R - R_t)
"""
import numpy as np

MAX_QUERIES = 256
QMETA_HDR = 4
QMETA_STRIDE = {"f16": 2, "f32": 2, "f8": 34}
TILE_ROWS = 32


def qblock_bytes(d_pad: int) -> int:
    return MAX_QUERIES * d_pad * 7 + 5 * 1024


def qblock_offsets(d_pad: int) -> dict:
    """Byte offset of every part of the query block."""
    nqd = MAX_QUERIES * d_pad
    return {"q32": 0, "q16": nqd * 4, "q8": nqd * 6, "eps16": nqd * 7, "eps8": nqd * 7 + 1024, "qinv": nqd * 7 + 2048,
            "hq": nqd * 7 + 3072, "floor": nqd * 7 + 4096}


def qblock_part(qblock_u8: np.ndarray, d_pad: int, name: str, nq: int) -> np.ndarray:
    """One part of a query block given as its bytes (uint8 [qblock_bytes(d_pad)]): the first nq queries of it."""
    off = qblock_offsets(d_pad)[name]
    qb = np.ascontiguousarray(qblock_u8, dtype=np.uint8)
    if name in ("q32", "q16", "q8"):
        dt = {"q32": np.float32, "q16": np.float16, "q8": np.int8}[name]
        n = MAX_QUERIES * d_pad * np.dtype(dt).itemsize
        return qb[off: off + n].view(dt).reshape(MAX_QUERIES, d_pad)[:nq]
    return qb[off: off + 1024].view(np.float32)[:nq]


def n_tiles(n_rows: int) -> int:
    return (n_rows + TILE_ROWS - 1) // TILE_ROWS


def qmeta_floats(n_rows: int, storage: str) -> int:
    return QMETA_HDR + QMETA_STRIDE[storage] * n_tiles(n_rows)


def tile_meta(qmeta: np.ndarray, n_rows: int, storage: str):
    """(s_t, R_t, 1/s_t) of every tile as float64 arrays [tiles], from the metadata floats."""
    stride, nt = QMETA_STRIDE[storage], n_tiles(n_rows)
    qm = np.ascontiguousarray(qmeta, dtype=np.float32)
    words = qm[QMETA_HDR: QMETA_HDR + stride * nt: stride].copy().view(np.uint32)
    s = (words & 0xffff).astype(np.uint16).view(np.float16).astype(np.float64)
    rt = (words >> 16).astype(np.uint16).view(np.float16).astype(np.float64)
    inv = qm[QMETA_HDR + 1: QMETA_HDR + 1 + stride * nt: stride].astype(np.float64)
    return s, rt, inv


def row_multipliers_f8(qmeta: np.ndarray, n_rows: int) -> np.ndarray:
    """fp8 rows: the multiplier of every stored row, float64 [n_rows]."""
    stride, nt = QMETA_STRIDE["f8"], n_tiles(n_rows)
    qm = np.ascontiguousarray(qmeta, dtype=np.float32)[QMETA_HDR: QMETA_HDR + stride * nt].reshape(nt, stride)
    return qm[:, 2:].reshape(-1)[:n_rows].astype(np.float64)


def tile_bounds(eps8: np.ndarray, hq: np.ndarray, R: float, rt: np.ndarray, n_rows: int) -> np.ndarray:
    """The per-tile form of the bound, one value per (query, row): eps8[q] - hq[q] * max(0, R - R_t(row))."""
    bonus = np.asarray(hq, np.float64)[:, None] * np.clip(float(R) - np.asarray(rt, np.float64), 0.0, None)[None, :]
    return np.repeat(np.asarray(eps8, np.float64)[:, None] - bonus, TILE_ROWS, axis=1)[:, :n_rows]


def check_bound(errs: np.ndarray, eps8: np.ndarray, hq: np.ndarray, R: float, rt: np.ndarray, attained: bool = True) -> float:
    """Assert both forms for the error matrix errs [nq][n_rows] (float64, |canonical - approx|); no tolerance.  R_t is an fp16
    rounded UP from a value <= R, so it may pass R by one fp16 step but no more, and the largest R_t is R itself — unless rows
    have been removed or a tile recomputed since (attained=False): R is only ever raised.  Returns the worst err / eps8."""
    errs = np.asarray(errs, np.float64)
    eps8 = np.asarray(eps8, np.float64)
    rt = np.asarray(rt, np.float64)
    assert np.isfinite(errs).all() and np.isfinite(eps8).all() and np.isfinite(rt).all(), "non-finite error or bound"
    # (one fp16 step: 2^-10 relative among normal halves, 2^-24 absolute among subnormal ones)
    assert (rt <= max(R * (1 + 2.0 ** -10), R + 2.0 ** -24)).all(), "a tile's R_t exceeds R by more than its rounding"
    assert not attained or float(rt.max()) >= float(R) * 0.999, "R is not attained by any tile"
    ratio = float((errs.max(axis=1) / eps8).max())
    assert (errs <= eps8[:, None]).all(), f"bound violated: worst err/eps8 = {ratio:.4f}"
    over = errs - tile_bounds(eps8, hq, R, rt, errs.shape[1])
    assert (over <= 0).all(), f"per-tile bound violated by {over.max():.3e} at (query, row) {np.unravel_index(over.argmax(), over.shape)}"
    return ratio


def int8_image_f16(rows_f16: np.ndarray, s_tile: np.ndarray) -> np.ndarray:
    """The int8 image of fp16 rows [n][d_pad] under the tile scales s_tile [tiles] (fp16-representable): d8 = the fp16
    fma(x, s, 1536) minus 1536.  In [1409, 1663] the fp16 step is 1, so the fma rounds the EXACT product x * s to the nearest
    integer, ties to even (1536 is even: the parity is d8's) — which is np.rint of the float64 product (22 bits: exact)."""
    x = np.asarray(rows_f16, np.float16).astype(np.float64)
    s = np.repeat(np.asarray(s_tile, np.float64), TILE_ROWS)[: x.shape[0]]
    d8 = np.rint(x * s[:, None])
    assert (np.abs(d8) <= 127).all()
    return d8.astype(np.int8)
