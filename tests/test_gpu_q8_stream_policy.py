"""The int8-prefilter scan's row stream (non-temporal row chunk loads, scan_q8.hip `fetch`) at the smallest shapes at which
the fetch path can go wrong.  Every case forces scan="q8", must return the oracle's ids and score bits, and must return
them again on a second search of the same index (the counted waits behind the prefetch are repeatable).

Rows: 1, 33 and 4001 leave almost every one of the 256 workgroups with nothing but the tile-0 redirect (4001 ends inside a
tile); 8193 rows = 257 tiles is the smallest shard in which workgroup 0 runs a second grid-stride iteration (tile 256), its
prefetch distance crossing the end.  Dimensions: 128 and 384 run four fetch groups (384 is the deep-D boundary), 768 is the
headline instantiation, 1024 recomputes its LDS offsets per use.  Storage: fp16, fp8 (768 and 1024), fp32 (scanned through
its fp16 image) and fp16 with the int8 shadow image; then the remaining instantiations whose machine code changed most (512 and
640 fp16, fp8 at 128 -> 256 and 512, shadow at 256 and 512).  One cascaded case: 2.1M rows is the smallest size at which the scan is
split (its 1/8 cut needs 16 pairs of tile rounds of 256 workgroups = 2,097,152 rows, rarc_scan_q8_launch), so the later
launches resume the candidate segments of the first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ, K = 256, 10
ROWS = (1, 33, 4001, 8193)
CONFIGS = ([("f16", False, d) for d in (128, 384, 768, 1024)] + [("f8", False, d) for d in (768, 1024)]
           + [("f32", False, d) for d in (128, 384, 768, 1024)] + [("f16", True, d) for d in (768, 1024)]
           # beyond the shapes above: the instantiations whose counted waits moved with the non-temporal load (<512,0>, <640,0>,
           # <256,1>: fp8 rows of 128 dimensions pad to 256, the four-group fp8 form) and the narrow fp8 / shadow forms
           + [("f16", False, d) for d in (512, 640)] + [("f8", False, d) for d in (128, 512)]
           + [("f16", True, d) for d in (256, 512)])
_refs = {}


def _reference(oracle, storage, n, d, nq=NQ, k=K, seed=None):
    """(X, Q, oracle ids, oracle scores) for 256 queries, computed once per shape and left unchanged; a search of the first
    nq queries must return the first nq rows (the canonical scorer treats every query on its own)."""
    key = (storage, n, d, nq, k)
    if key not in _refs:
        rng = np.random.default_rng(1000 * d + n if seed is None else seed)
        X = rng.standard_normal((n, d), dtype=np.float32)
        Q = rng.standard_normal((nq, d), dtype=np.float32)
        qn = oracle.normalize_L2(Q)
        kk = min(k, n)
        if storage == "f8":
            b, s, _ = oracle.ingest_f8(X)
            I, D = oracle.flat_search_f8(b, s, qn, kk)[:2]
        elif storage == "f32":
            I, D = oracle.flat_search_f32(oracle.ingest_f32(X)[0], qn, kk)[:2]
        else:
            I, D = oracle.flat_search_f16(oracle.ingest_f16(X)[0], qn, kk)[:2]
        _refs[key] = (X, Q, I, D)
    return _refs[key]


def _check(idx, Q, kk, ref_I, ref_D, what):
    D, I = idx.search(Q, kk)
    assert np.array_equal(I, ref_I), f"{what}: ids differ from the oracle"
    assert np.array_equal(D.view(np.uint32), ref_D.view(np.uint32)), f"{what}: score bits differ from the oracle"
    D2, I2 = idx.search(Q, kk)
    assert np.array_equal(I2, I) and np.array_equal(D2.view(np.uint32), D.view(np.uint32)), f"{what}: a second search differs"


@pytest.mark.parametrize("nq", (1, NQ))
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("storage,shadow,d", CONFIGS)
def test_row_stream_matches_oracle(oracle, storage, shadow, d, n, nq):
    from rag_arc_amd.hip.engine import FlatIndexF16

    X, Q, ref_I, ref_D = _reference(oracle, storage, n, d)
    idx = FlatIndexF16(d, metric="cosine", scan="q8", storage=storage, shadow=shadow)
    idx.add(X)
    _check(idx, Q[:nq], min(K, n), ref_I[:nq], ref_D[:nq], f"{storage}{' + shadow' if shadow else ''} n={n} d={d} nq={nq}")


def test_row_stream_cascaded_scan(oracle):
    """2.1M x 128 fp16 rows, 256 queries, k = 100: the scan is split, every launch after the first resumes."""
    from rag_arc_amd.hip.engine import FlatIndexF16

    n, d, k = 2_100_000, 128, 100
    assert (n + 31) // 32 // 8 // 512 * 512 >= 16 * 512, "the 1/8 cut needs 16 pairs of tile rounds"
    X, Q, ref_I, ref_D = _reference(oracle, "f16", n, d, k=k, seed=2100)
    idx = FlatIndexF16(d, metric="cosine", scan="q8")
    idx.add(X)
    _check(idx, Q, k, ref_I, ref_D, f"cascaded n={n} d={d}")
    # and the scan really was split: the library brackets every scan launch of a profiled search
    import ctypes

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    B.check(lib.rarc_profile_begin(64))
    idx.search(Q, k)
    tot, launches = ctypes.c_double(0), ctypes.c_int(0)
    B.check(lib.rarc_profile_end(ctypes.byref(tot), ctypes.byref(launches)))
    assert launches.value >= 2, f"{launches.value} scan launch(es): the cascade did not cut, no launch resumed"
