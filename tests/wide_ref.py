"""Host restatement of the wide search path (csrc/wide.hip), numpy only, for the tests that aim at one of its forms
(tests/test_gpu_wide_forms.py) or at its pruning bound (tests/test_gpu_wide_bound.py); held to hand-made examples and to the
ladder's own rules in tests/test_wide_ref_host.py.

plan(n, k, d_pad): the chunk plan of wide_search_impl in the default environment (RARC_WIDE_FUSE, RARC_WIDE_SMALL_TILES and
RARC_WIDE_FUSED_ROWS unset), one Piece per launch group, in order:
    first      rows [0, first): GEMM into the score buffer, every row a candidate of every query (wide_select_kernel, first = 1)
    fused128   a later chunk nominated in the epilogue of the 128 x 128 ping-pong GEMM (at most 256 tiles of 256 rows)
    fused256   the same in the 256 x 256 kernel (more than 65536 rows)
    stored     a later chunk through the score buffer: GEMM, then wide_select_kernel against the thresholds (first = 0)
`tail` says the piece ends in the zero-padded 128-row block (its row count is no multiple of 128).  The fused GEMM takes whole
256-row blocks of rows with d_pad >= 256; the first chunk absorbs (n - 16384) % 256, so every later chunk is a multiple of 256
and rows narrower than 256 padded dimensions are the only ones whose later chunks are `stored`.

The float64 helpers restate the two sides of the bound: dot64 (the exact inner product of the fp16 query with the fp16 row or
image, which the approximate score differs from by accumulation and fp16-store error only) and the k-th best values the
thresholds are held against."""
from collections import namedtuple

import numpy as np

MAX_QUERIES = 256
WIDE_CHUNK = 131072            # rows per GEMM that stores its scores
WIDE_FUSED_CHUNK = 1 << 20     # rows per GEMM that nominates in its epilogue
WIDE_KMAX = 8192
SMALL_TILES_MAX = 256          # 256-row tiles the 128 x 128 kernel takes; beyond: the 256 x 256 kernel
TIGHTEN_LDS_KEYS = 20480       # list entries the tighten pass selects on in LDS; beyond: the streaming form

Piece = namedtuple("Piece", "start rows form tail")


def fused_takes(m: int, d_pad: int) -> bool:
    """rarc_gemm_f16_select_takes: whole 256-row blocks, K a multiple of 64 and at least 256."""
    return m > 0 and m % 256 == 0 and d_pad % 64 == 0 and d_pad >= 256


def first_rows(k: int) -> int:
    return (max(16384, 2 * k) + 255) // 256 * 256


def plan(n: int, k: int, d_pad: int):
    """The pieces of one rarc_search_wide / rarc_search_wide_l2 call over n rows, in launch order."""
    assert n >= 0 and 1 <= k <= WIDE_KMAX and d_pad > 0 and d_pad % 128 == 0 and d_pad <= 4096
    first = first_rows(k)
    growth = 4 if k <= 1024 else 2
    chunk = first + (n - first) % 256 if n > first else n
    nominal, at, out = first, 0, []
    while at < n:
        m = min(n - at, chunk)
        if at > 0 and m >= 256 and fused_takes(m // 256 * 256, d_pad):
            mf = m // 256 * 256
            out.append(Piece(at, mf, "fused128" if mf // 256 <= SMALL_TILES_MAX else "fused256", False))
            at += mf
            m -= mf
            if m == 0:
                nominal = min(nominal * growth, WIDE_FUSED_CHUNK)
                chunk = nominal
                continue
        if m > WIDE_CHUNK:
            chunk = m = WIDE_CHUNK
        out.append(Piece(at, m, "first" if at == 0 else "stored", m % 128 != 0))
        at += m
        nominal = min(nominal * growth, WIDE_FUSED_CHUNK)
        chunk = min(nominal, WIDE_CHUNK)
    return out


def forms(n: int, k: int, d_pad: int):
    return [p.form for p in plan(n, k, d_pad)]


def smallest_n_with(wanted, k: int, d_pad: int, limit: int = 1 << 21) -> int:
    """The smallest n whose plan holds every form of `wanted` (later chunks come in steps of 256 rows)."""
    n = first_rows(k)
    while n <= limit:
        if set(wanted) <= set(forms(n, k, d_pad)):
            return n
        n += 256
    raise ValueError(f"no n <= {limit} reaches {wanted}")


# ---- the bound, in float64 ---------------------------------------------------------------------------------------------
def dot64(q16: np.ndarray, x16: np.ndarray, block: int = 4096) -> np.ndarray:
    """[nq][n] float64 inner products of fp16 queries with fp16 rows (products exact, sums within 1e-13 relative of |q||x|)."""
    q = np.asarray(q16, np.float16).astype(np.float64)
    out = np.empty((q.shape[0], x16.shape[0]), np.float64)
    for s in range(0, x16.shape[0], block):
        out[:, s:s + block] = q @ np.asarray(x16[s:s + block], np.float16).astype(np.float64).T
    return out


def image16(rows: np.ndarray) -> np.ndarray:
    """What the score GEMM reads: fp16 rows as they are (uint16 bit patterns), fp32 rows rounded to nearest even."""
    rows = np.asarray(rows)
    return rows.view(np.float16) if rows.dtype == np.uint16 else rows.astype(np.float16)


def kth_largest(a: np.ndarray, k: int) -> np.ndarray:
    """Per row of a [nq][n]: the k-th largest value (k <= n)."""
    a = np.asarray(a)
    return np.partition(a, a.shape[1] - k, axis=1)[:, a.shape[1] - k]


def l2_kappa(ip: np.ndarray, xn: np.ndarray) -> np.ndarray:
    """kappa = ip - xn / 2 in float64 from the canonical fp32 ip [nq][n] and the stored fp32 squared norms xn [n]."""
    return np.asarray(ip, np.float32).astype(np.float64) - 0.5 * np.asarray(xn, np.float32).astype(np.float64)[None, :]


def l2_dist_error(dist: np.ndarray, qn: np.ndarray, kappa: np.ndarray) -> np.ndarray:
    """Per query: max over rows of |dist - max(0, qn - 2 kappa)| — what delta of the header of csrc/wide.hip has to cover
    (dist the fp32 distances of tests/l2_ref.py, qn the canonical fp32 |q|^2)."""
    real = np.maximum(0.0, np.asarray(qn, np.float32).astype(np.float64)[:, None] - 2.0 * kappa)
    return np.abs(np.asarray(dist, np.float32).astype(np.float64) - real).max(axis=1)
