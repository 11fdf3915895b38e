"""Every chunk form of the wide search (csrc/wide.hip) against the oracle: ids and score bits, as in tests/test_gpu_wide.py
and tests/test_gpu_l2.py, at shapes chosen so that a named form runs — and tests/wide_ref.py's plan() asserts that it does,
so a change to the chunk ladder fails here instead of emptying a test.

  stored later chunks  wide_select_kernel with a live threshold (fp16 pre-screen, dead groups, four rows in flight + the
                       remainder loop; under "l2" the key from xn[row0 + r]).  A later chunk stays out of the fused GEMM only
                       when d_pad < 256, and rows are padded to a multiple of 128: d <= 128.  d = 192 pads to 256 and runs the
                       fused form; it is kept next to d = 64 and d = 128 and its plan asserted for what it is.
  first chunk / tail   n around 16384 and around the 128- and 256-row blocks behind it (d = 256: fused afterwards)
  fused kernels        the 128 x 128 and the 256 x 256 select GEMM in one search; k = 8192 on 60k rows (the tighten's
                       streaming form); exact duplicates in the first and in the last chunk (the id decides)
"""
import functools

import numpy as np
import pytest

from tests import l2_ref
from tests import wide_ref as WR

pytestmark = pytest.mark.gpu

FIRST = 16384


@pytest.fixture(scope="module")
def hip():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from rag_arc_amd.hip import engine

    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ip_reference(oracle, X, Q, k, metric, storage):
    """(D, I) of the oracle for cosine / ip at the largest k asked for (a smaller k is its prefix: the order is total)."""
    qn = oracle.normalize_L2(Q) if metric == "cosine" else Q
    if storage == "f32":
        I, D = oracle.flat_search_f32(oracle.ingest_f32(X, normalize=(metric == "cosine"))[0], qn, k)[:2]
    else:
        I, D, _ = oracle.flat_search_f16(oracle.ingest_f16(X, normalize=(metric == "cosine"))[0], qn, k)
    return D, I


def _check(hip, oracle, X, Q, metric, storage, ks, what):
    """Search at every k of ks and compare ids and score bits with the reference; returns the reference at max(ks)."""
    idx = hip.FlatIndexF16(X.shape[1], metric=metric, storage=storage)
    idx.add(X)
    kmax = max(ks)
    if metric == "l2":
        ref_D, ref_I = l2_ref.search(oracle, X, Q, kmax, storage)
    else:
        ref_D, ref_I = _ip_reference(oracle, X, Q, kmax, metric, storage)
    for k in ks:
        assert idx._takes_wide_path(k), (metric, k)
        D, I = idx.search(Q, k)
        bad = [q for q in range(Q.shape[0]) if not (np.array_equal(I[q], ref_I[q, :k]) and
                                                    np.array_equal(_bits(D[q]), _bits(ref_D[q, :k])))]
        assert not bad, f"{what} {metric} {storage} k={k}: queries {bad[:8]} differ from the oracle"
    return ref_D, ref_I


@functools.lru_cache(maxsize=2)
def _planted(n, d, nq=6):
    """Gaussian rows with norms over 0.5 .. 2 and, per query, one row at 1.5 x the query: the best row under every metric —
    of the even queries in the LAST chunk (rows n - 1 - j), of the odd ones in the first (rows j)."""
    rng = np.random.default_rng(n * 1000 + d)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X *= np.exp2(rng.uniform(-1, 1, (n, 1))).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32) * np.float32(2.5)
    where = [n - 1 - j if j % 2 == 0 else j for j in range(nq)]
    for j, r in enumerate(where):
        X[r] = Q[j] * np.float32(1.5)
    return X, Q, where


STORED_N = (FIRST + 1, FIRST + 255, FIRST + 256, FIRST + 257, FIRST + 65536 + 256 + 77, 90_001)
STORED_CASES = [(n, d, ("f16", "f32")[(i + j) % 2]) for i, n in enumerate(STORED_N) for j, d in enumerate((64, 128, 192))]


@pytest.mark.parametrize("n,d,storage", STORED_CASES)
def test_later_chunks_through_the_score_buffer(hip, oracle, n, d, storage):
    d_pad = oracle.padded_dim(d)
    for k in (1, 10, 1000, 1025, 4000):
        later = WR.forms(n, k, d_pad)[1:]
        if d_pad < 256:       # the premise: every later chunk is GEMM + wide_select_kernel against the thresholds
            assert later == ["stored"] * len(later) and (len(later) > 0) == (n - FIRST >= 256), (n, k, later)
        else:                 # d = 192 pads to 256: the fused GEMM takes these
            assert all(f.startswith("fused") for f in later)
    if d_pad < 256:
        assert len(WR.forms(90_001, 1025, d_pad)) == 3 and len(WR.forms(FIRST + 65536 + 256 + 77, 10, d_pad)) == 3
    X, Q, where = _planted(n, d)
    for metric, ks in (("cosine", (1025, 4000)), ("ip", (1025, 4000)), ("l2", (1, 10, 1000, 4000))):
        _, ref_I = _check(hip, oracle, X, Q, metric, storage, ks, f"n={n} d={d}")
        assert ref_I[:, 0].tolist() == where, (metric, "the planted rows are the best ones")


@pytest.mark.parametrize("nq", [1, 9, 255, 256])
def test_ragged_query_blocks_on_stored_chunks(hip, oracle, nq):
    """The select pass decides `dead` per group of 8 queries from two of its thresholds: nq = 1 and 9 leave a group with one
    live query, 255 a group with one padding query, 256 none."""
    n, d = FIRST + 512 + 77, 64
    assert WR.forms(n, 1025, 128) == ["first", "stored"] and WR.forms(n, 10, 128) == ["first", "stored"]
    rng = np.random.default_rng(nq)
    X = rng.standard_normal((n, d)).astype(np.float32) * np.exp2(rng.uniform(-1, 1, (n, 1))).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    X[n - nq:] = Q * np.float32(1.5)                     # every query's best row sits in the later chunk
    _, ref_I = _check(hip, oracle, X, Q, "cosine", "f16", (1025,), f"nq={nq}")
    assert ref_I[:, 0].tolist() == list(range(n - nq, n))
    _check(hip, oracle, X, Q, "l2", "f16", (10,), f"nq={nq}")


def _column_scores(rng, n, k, values):
    """A column whose k - 1 largest entries are clearly positive, then `values` repeated over a few thousand rows of both
    chunks, the rest clearly negative — so the k-th best entry is one of `values`."""
    col = -rng.uniform(0.25, 1.0, n)
    order = rng.permutation(n)
    col[order[:k - 1]] = rng.uniform(0.25, 1.0, k - 1)
    mid = order[k - 1:k - 1 + 3000]
    col[mid] = rng.choice(values, 3000)
    return col


def test_negative_and_subnormal_kth_best_on_a_stored_chunk(hip, oracle):
    """Metric "ip", d = 64, k = 8192 of 16384 + 1024 rows, queries along the axes, so a row's score is one of its elements.
    Queries 0..3: the k-th best score is negative (most rows score below zero and the threshold the later chunk is screened
    with is negative).  Queries 4..7, of norm 2^-10: the k-th best is a multiple of 2^-24 within 8 steps of zero (an fp16
    subnormal), tied over a hundred and more rows of both chunks, and eps is a few dozen such steps: the fp16 pre-screen works
    on subnormal thresholds."""
    n, d, k = FIRST + 1024, 64, 8192
    assert WR.forms(n, k, 128) == ["first", "stored"]
    rng = np.random.default_rng(77)
    X = (rng.standard_normal((n, d)) * 0.02).astype(np.float32)
    Q = np.zeros((8, d), np.float32)
    for j in range(4):
        X[:, j] = _column_scores(rng, n, k, -np.arange(1, 40) / 256.0)
        Q[j, j] = 1.0
    for j in range(4, 8):
        X[:, j] = _column_scores(rng, n, k, np.arange(-8, 9) * 2.0 ** -14)
        Q[j, j] = 2.0 ** -10
    X = X.astype(np.float16).astype(np.float32)
    ref_D, ref_I = _check(hip, oracle, X, Q, "ip", "f16", (k,), "negative / subnormal k-th best")
    assert (ref_D[:4, k - 1] < -1e-3).all(), "queries 0..3: the k-th best score is negative"
    assert (np.abs(ref_D[4:, k - 1]) <= 8 * 2.0 ** -24).all(), "queries 4..7: the k-th best is within 8 fp16 subnormal steps of 0"
    for q in range(8):       # and the tie on it spans both chunks
        tied = np.nonzero(X[:, q] * Q[q, q] == ref_D[q, k - 1])[0]
        assert tied.min() < FIRST <= tied.max()


BOUNDARY_N = (FIRST - 1, FIRST, FIRST + 1, FIRST + 127, FIRST + 128, FIRST + 255, FIRST + 256, FIRST + 257, FIRST + 512 + 129)


@pytest.mark.parametrize("n", BOUNDARY_N)
def test_first_chunk_and_tail_boundaries(hip, oracle, n):
    d = 256
    pieces = WR.plan(n, 1025, d)
    assert pieces == WR.plan(n, 8192, d)
    assert pieces[0].rows == (n if n < FIRST + 256 else FIRST + (n - FIRST) % 256) and pieces[0].tail == (pieces[0].rows % 128 != 0)
    assert [p.form for p in pieces[1:]] == (["fused128"] if n >= FIRST + 256 else [])
    X, Q, _ = _planted(n, d, nq=5)
    _check(hip, oracle, X, Q, "cosine", "f16", (1025, 8192), f"n={n}")
    _check(hip, oracle, X, Q, "l2", "f16", (1025, 8192), f"n={n}")


@pytest.mark.parametrize("metric,k", [("cosine", 1025), ("l2", 100)])
def test_both_fused_kernels_in_one_search(hip, oracle, metric, k):
    """The smallest corpus of d = 256 whose plan holds a chunk of the 128 x 128 select GEMM and one of the 256 x 256 kernel
    (k <= 1024 quadruples its chunks and gets there at 147,712 rows; cosine needs k > 1024 for this path and doubles)."""
    d = 256
    n = WR.smallest_n_with(("fused128", "fused256"), k, d)
    assert n == {100: 147_712, 1025: 180_480}[k]
    forms = WR.forms(n, k, d)
    assert forms[0] == "first" and "fused128" in forms and forms[-1] == "fused256" and "stored" not in forms
    X, Q, where = _planted(n, d)
    _, ref_I = _check(hip, oracle, X, Q, metric, "f16", (k,), f"n={n}")
    assert ref_I[:, 0].tolist() == where


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_k_8192_streams_the_tighten(hip, oracle, metric):
    """k = 8192 on 59,469 rows of d = 256: chunks of 16,384 + 77, 32,768 and 10,240 rows.  The threshold behind the first
    chunk is its 8192nd best score less the margin — about its median — so about half of the second chunk is nominated (the
    ladder's own estimate: ~2k nominations per doubling) and the tighten behind it selects on a list of more than 20,480
    entries, which is its streaming form (wide_kth_largest_each); the other two tighten passes fit LDS.
    The list counts before a tighten are not kept by the search, so that count is not read back and asserted.  What is
    asserted is its lower bound from the oracle: a row of the second chunk at least as good as the first chunk's k-th best is
    a candidate whatever the margin, and the list holds at least k entries of the first chunk besides."""
    n, d, k = FIRST + 32768 + 10240 + 77, 256, 8192
    pieces = WR.plan(n, k, d)
    assert [(p.rows, p.form) for p in pieces] == [(FIRST + 77, "first"), (32768, "fused128"), (10240, "fused128")]
    X, Q, _ = _planted(n, d, nq=5)
    a, b = pieces[1].start, pieces[2].start
    if metric == "l2":
        dist = l2_ref.distances(oracle, l2_ref.stored_rows(oracle, X), Q)[0]
        sure = (dist[:, a:b] <= np.sort(dist[:, :a], axis=1)[:, k - 1:k]).sum(axis=1)
    else:
        rows = oracle.ingest_f16(X, normalize=True)[0]
        sc = l2_ref.all_dots(oracle, rows, oracle.pad_queries(oracle.normalize_L2(Q), d))
        sure = (sc[:, a:b] >= WR.kth_largest(sc[:, :a], k)[:, None]).sum(axis=1)
    print(f"k=8192 {metric}: entries the second tighten selects on >= {(k + sure).tolist()}")
    assert (k + sure > WR.TIGHTEN_LDS_KEYS).all()
    _check(hip, oracle, X, Q, metric, "f16", (k,), "k=8192")


@pytest.mark.parametrize("d", [64, 256])
def test_exact_duplicates_in_the_first_and_the_last_chunk(hip, oracle, d):
    """Bit-equal rows in the first chunk, in a middle one and in the last one; query 0 is that row, query 1 another
    duplicated row.  Equal canonical scores: the id decides, across chunks — under "l2" three copies at distance 0."""
    n = FIRST + 32768 + 4096 + 33
    later = WR.forms(n, 1025, oracle.padded_dim(d))[1:]
    assert later == [("stored" if d < 256 else "fused128")] * 2 and WR.forms(n, 10, oracle.padded_dim(d))[1:] == later[:1]
    rng = np.random.default_rng(d)
    X = rng.standard_normal((n, d)).astype(np.float32).astype(np.float16).astype(np.float32)
    copies = [[5, 30_000, n - 3], [16_000, 50_000, n - 1]]
    for c in copies:
        X[c[1]] = X[c[0]]
        X[c[2]] = X[c[0]]
    Q = np.concatenate([X[[5, 16_000]], rng.standard_normal((3, d)).astype(np.float32)])
    for metric, k in (("cosine", 1025), ("ip", 1025), ("l2", 10)):
        ref_D, ref_I = _check(hip, oracle, X, Q, metric, "f16", (k,), f"duplicates d={d}")
        for q, c in enumerate(copies):
            assert ref_I[q, :3].tolist() == c and len(set(_bits(ref_D[q, :3]).tolist())) == 1
            assert metric != "l2" or (ref_D[q, :3] == 0.0).all()
