"""The edge of the fp16 range, metric "ip" (cosine rows and queries are normalised and cannot get there).  Rows stored as
fp32 are scanned through an fp16 image, every narrow-path query has an fp16 copy (q16), and the wide path keeps fp16 scores:
an element of 65520 or more has no finite fp16, and a score may pass 65504 with ordinary elements.

The contract, for every case here: the answer is the oracle's, ids and score bits — or RarcUnsupported is raised before the
rows or queries reach a search kernel (at add or at search), its message says what does answer, and the index is as usable
as before.  Never an infinity, a NaN or another id set."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE = [65504.0, 65519.0, 65520.0, 1e5, 1e30]       # the largest fp16; the last fp32 that rounds to it; the first that does
#                                                     not; beyond; far beyond
N, NQ, K = 2000, 4, 10


def _oracle_search(oracle, storage, X, Q, k):
    if storage == "f16":
        return oracle.flat_search_f16(oracle.ingest_f16(X, normalize=False)[0], Q, k)[:2]
    if storage == "f8":
        b8, s8, _ = oracle.ingest_f8(X, normalize=False)
        return oracle.flat_search_f8(b8, s8, Q, k)[:2]
    return oracle.flat_search_f32(oracle.ingest_f32(X, normalize=False)[0], Q, k)[:2]


def _index(storage, d, scan="auto"):
    from rag_arc_amd.hip.engine import FlatIndexF16

    return FlatIndexF16(d, metric="ip", storage=storage, scan=scan)


def _same(D, I, ref):
    assert np.array_equal(I, ref[0]), "ids differ from the oracle's"
    assert np.array_equal(D.view(np.uint32), ref[1].view(np.uint32)), "score bits differ from the oracle's"


def _refusal(exc):
    msg = str(exc)
    assert "scale" in msg and ("cosine" in msg or "f16" in msg or "f32" in msg), f"the refusal names no way out: {msg}"
    return "refused"


def _answer_or_refusal(oracle, idx, storage, X, Q, k, plain_X, plain_Q):
    """Run add + search under the contract.  plain_X / plain_Q: ordinary data the index must still answer on afterwards."""
    from rag_arc_amd.hip import binding as B

    ref = _oracle_search(oracle, storage, X, Q, k)
    held = plain_X
    try:
        idx.add(X)
        held = X
        D, I = idx.search(Q, k)
    except B.RarcUnsupported as exc:
        outcome = _refusal(exc)
    else:
        assert np.isfinite(D).all()
        _same(D, I, ref)
        outcome = "exact"
    if outcome == "refused":                        # left usable: nothing of the refused call stays behind
        if held is plain_X:
            assert idx.ntotal == 0
            idx.add(plain_X)
        assert idx.ntotal == len(held)
        D, I = idx.search(plain_Q, k)
        _same(D, I, _oracle_search(oracle, storage, held, plain_Q, k))
    return outcome


def _data(d, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((NQ, d)).astype(np.float32), rng


@pytest.mark.parametrize("d", [256, 1536])
def test_fp32_rows_with_elements_at_the_fp16_limit(oracle, d):
    """One planted row per query: an element of the edge value, signed like the query's, in a column where the query is
    large — the planted row is that query's best by far, which the oracle confirms before the GPU is asked."""
    X0, Q, rng = _data(d, 7)
    outcomes = {}
    for v in EDGE:
        X = X0.copy()
        planted = rng.choice(N, NQ, replace=False)
        for j, r in enumerate(planted):
            col = int(np.abs(Q[j]).argmax())
            X[r, col] = np.float32(v) * np.sign(Q[j, col])
        ref = _oracle_search(oracle, "f32", X, Q, K)
        assert np.array_equal(ref[0][:, 0], planted) and np.isfinite(ref[1]).all() and float(ref[1].max()) > v
        outcomes[v] = _answer_or_refusal(oracle, _index("f32", d), "f32", X, Q, K, X0, Q)
    print(f"fp32 rows d={d}:", outcomes)
    assert outcomes[65504.0] == outcomes[65519.0] == "exact", "elements with a finite fp16 image are in range"


NARROW = [("f16", "q8"), ("f16", "mfma16"), ("f16", "auto"), ("f8", "auto"), ("f32", "auto")]


@pytest.mark.parametrize("storage, scan, d", [(s, c, 256) for s, c in NARROW] + [("f16", "auto", 1536), ("f32", "auto", 1536)])
def test_queries_with_elements_at_the_fp16_limit(oracle, storage, scan, d):
    """Ordinary rows; every query carries one edge value."""
    X, Q0, rng = _data(d, 8)
    idx = _index(storage, d, scan)
    idx.add(X)
    outcomes = {}
    for v in EDGE:
        Q = Q0.copy()
        Q[np.arange(NQ), rng.integers(0, d, NQ)] = np.float32(v) * rng.choice([-1.0, 1.0], NQ).astype(np.float32)
        ref = _oracle_search(oracle, storage, X, Q, K)
        assert np.isfinite(ref[1]).all() and float(ref[1].max()) > v / 2
        from rag_arc_amd.hip import binding as B

        try:
            D, I = idx.search(Q, K)
        except B.RarcUnsupported as exc:
            outcomes[v] = _refusal(exc)
        else:
            assert np.isfinite(D).all(), f"query element {v}: non-finite scores"
            _same(D, I, ref)
            outcomes[v] = "exact"
        print(f"queries {storage} {scan} d={d} element {v}: {outcomes[v]}")
        D, I = idx.search(Q0, K)                    # and the index answers ordinary queries as before
        _same(D, I, _oracle_search(oracle, storage, X, Q0, K))
    assert outcomes[65504.0] == outcomes[65519.0] == "exact", "elements with a finite fp16 copy are in range"


@pytest.mark.parametrize("storage, scan, d", [(s, c, 256) for s, c in NARROW] + [("f16", "auto", 1536), ("f32", "auto", 1536)])
def test_scores_beyond_the_fp16_range_from_ordinary_elements(oracle, storage, scan, d):
    """||q|| * ||row|| > 65504 with no element anywhere near the limit: rows of norm 500, queries of norm 400, and for every
    query one row parallel to it (score 2e5), planted in the last tile."""
    X, Q, rng = _data(d, 9)
    X *= np.float32(500.0 / np.sqrt(d))
    Q *= np.float32(400.0 / np.sqrt(d))
    for j in range(NQ):
        X[N - 1 - j] = Q[j] / np.linalg.norm(Q[j]) * 500.0
    assert np.abs(X).max() < 4096 and np.abs(Q).max() < 4096
    ref = _oracle_search(oracle, storage, X, Q, K)
    assert float(ref[1][:, 0].min()) > 65504.0 and [int(i) for i in ref[0][:, 0]] == [N - 1 - j for j in range(NQ)]
    plain = (X / np.float32(64.0)).astype(np.float32)
    print(f"scores {storage} {scan} d={d}:", _answer_or_refusal(oracle, _index(storage, d, scan), storage, X, Q, K, plain, Q / np.float32(64.0)))
