"""The int8-prefilter scan with the threshold / histogram refresh once per loop unit (scan_q8.hip: Q8_RF_FETCH), at the
smallest shapes at which it can go wrong.  Every case forces scan="q8",
must return the oracle's ids and score bits, and must return them again on a second search of the same index.

Rows: 1, 33 and 4001 leave almost every one of the 256 workgroups with nothing but the tile-0 redirect; 8193 rows = 257 tiles is the smallest shard in which workgroup 0 runs a
second grid-stride iteration.  Dimensions: 128 and 384 run four fetch groups (refresh in group 1, as before), 768 two (now
group 1 only), 1024 fp16 one (now every second iteration, by the parity of the unrolled pair); fp8 and int8-shadow rows exist at
multiples of 256 only, so they run 256 (four groups), 512, 768 and 1024.  fp32 rows are scanned through their fp16 image.
Queries 1 / 255 / 256 and k 1 / 100 share one index per shape.

Two planted shards where the feedback matters (8193 x 768 fp16, every query close to one common direction, the planted rows
closer to it than any other row): planted in the LAST tiles, the threshold can only rise late and by the histogram; planted
in tile 0, it is final before the first refresh.  Exact answers, and no query repaired.

One cascaded case (2.1M x 128: the smallest shard the cascade cuts), which asserts that the scan ran as more than one launch."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NQ = 256
ROWS = (1, 33, 4001, 8193)
KS = (1, 100)
NQS = (1, 255, 256)
CONFIGS = ([("f16", False, d) for d in (128, 384, 768, 1024)] + [("f32", False, d) for d in (128, 384, 768, 1024)]
           + [("f8", False, d) for d in (256, 512, 768, 1024)] + [("f16", True, d) for d in (256, 512, 768, 1024)])
_refs = {}


def _oracle_topk(oracle, storage, X, Q, k):
    qn = oracle.normalize_L2(Q)
    if storage == "f8":
        b, s, _ = oracle.ingest_f8(X)
        return oracle.flat_search_f8(b, s, qn, k)[:2]
    if storage == "f32":
        return oracle.flat_search_f32(oracle.ingest_f32(X)[0], qn, k)[:2]
    return oracle.flat_search_f16(oracle.ingest_f16(X)[0], qn, k)[:2]


def _reference(oracle, storage, n, d):
    """(X, Q, {k: (oracle ids, oracle scores)}) for 256 queries, computed once per shape and left unchanged; a search of the
    first nq queries must return the first nq rows (the canonical scorer treats every query on its own)."""
    key = (storage, n, d)
    if key not in _refs:
        rng = np.random.default_rng(3000 * d + n)
        X = rng.standard_normal((n, d), dtype=np.float32)
        Q = rng.standard_normal((NQ, d), dtype=np.float32)
        _refs[key] = (X, Q, {k: _oracle_topk(oracle, storage, X, Q, min(k, n)) for k in KS})
    return _refs[key]


def _check(idx, Q, kk, ref_I, ref_D, what):
    D, I = idx.search(Q, kk)
    assert np.array_equal(I, ref_I), f"{what}: ids differ from the oracle"
    assert np.array_equal(D.view(np.uint32), ref_D.view(np.uint32)), f"{what}: score bits differ from the oracle"
    D2, I2 = idx.search(Q, kk)
    assert np.array_equal(I2, I) and np.array_equal(D2.view(np.uint32), D.view(np.uint32)), f"{what}: a second search differs"


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("storage,shadow,d", CONFIGS)
def test_refresh_matches_oracle(oracle, storage, shadow, d, n):
    from rag_arc_amd.hip.engine import FlatIndexF16

    X, Q, refs = _reference(oracle, storage, n, d)
    idx = FlatIndexF16(d, metric="cosine", scan="q8", storage=storage, shadow=shadow)
    idx.add(X)
    for k in KS:
        ref_I, ref_D = refs[k]
        for nq in NQS:
            _check(idx, Q[:nq], min(k, n), ref_I[:nq], ref_D[:nq],
                   f"{storage}{' + shadow' if shadow else ''} n={n} d={d} nq={nq} k={k}")


def _planted(where, n_plant):
    """8193 x 768 rows; the queries are one common direction plus a little of their own, the planted rows are that direction
    plus less: every planted row beats every other row for every query (cosine ~0.9 against ~0.04 at most)."""
    n, d = 8193, 768
    rng = np.random.default_rng(76800 + n_plant + (1 if where == "last" else 0))
    c = rng.standard_normal(d).astype(np.float32)
    c /= np.linalg.norm(c)
    Q = (c[None, :] + 0.3 * rng.standard_normal((NQ, d), dtype=np.float32) / np.sqrt(d)).astype(np.float32)
    X = rng.standard_normal((n, d), dtype=np.float32)   # (scores around 0)
    P =(c[None, :] + 0.4 * rng.standard_normal((n_plant, d), dtype=np.float32) / np.sqrt(d)).astype(np.float32)
    lo = 0 if where == "tile0" else n - n_plant
    X[lo:lo + n_plant] = P * np.float32(np.sqrt(d))   # (norms like the other rows': cosine normalises them anyway)
    return X, Q, lo


@pytest.mark.parametrize("where,n_plant,k", (("last", 160, 100), ("last", 160, 1), ("tile0", 32, 10), ("tile0", 32, 1)))
def test_refresh_planted_rows(oracle, where, n_plant, k):
    from rag_arc_amd.hip.engine import FlatIndexF16

    X, Q, lo = _planted(where, n_plant)
    ref_I, ref_D = _oracle_topk(oracle, "f16", X, Q, k)
    assert ((ref_I >= lo) & (ref_I < lo + n_plant)).all(), "the planted rows are not every query's top-k"
    idx = FlatIndexF16(768, metric="cosine", scan="q8")
    idx.add(X)
    for r in range(2):
        D, I = idx.search(Q, k)
        what = f"planted in {where}, k={k}, search {r + 1}"
        assert np.array_equal(I, ref_I), f"{what}: ids differ from the oracle"
        assert np.array_equal(D.view(np.uint32), ref_D.view(np.uint32)), f"{what}: score bits differ from the oracle"
        assert len(idx.last_repaired) == 0, f"{what}: repaired queries {list(idx.last_repaired)[:8]}"


def test_refresh_cascaded_scan(oracle):
    """2.1M x 128 fp16 rows, 256 queries, k = 100: the scan is split, every launch after the first resumes."""
    from rag_arc_amd.hip import binding as B
    from rag_arc_amd.hip.engine import FlatIndexF16

    n, d, k = 2_100_000, 128, 100
    rng = np.random.default_rng(2101)
    X = rng.standard_normal((n, d), dtype=np.float32)
    Q = rng.standard_normal((NQ, d), dtype=np.float32)
    ref_I, ref_D = _oracle_topk(oracle, "f16", X, Q, k)
    idx = FlatIndexF16(d, metric="cosine", scan="q8")
    idx.add(X)
    _check(idx, Q, k, ref_I, ref_D, f"cascaded n={n} d={d}")
    assert len(idx.last_repaired) == 0, f"cascaded: repaired queries {list(idx.last_repaired)[:8]}"
    lib = B.load_library()
    B.check(lib.rarc_profile_begin(64))
    idx.search(Q, k)
    tot, launches = ctypes.c_double(0), ctypes.c_int(0)
    B.check(lib.rarc_profile_end(ctypes.byref(tot), ctypes.byref(launches)))
    assert launches.value >= 2, f"{launches.value} scan launch(es): the cascade did not cut, no launch resumed"
