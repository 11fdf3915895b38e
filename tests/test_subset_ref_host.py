"""The filtered search's CPU side (no GPU): the restatement tests/subset_ref.py equals the oracle's full ranking with the
disallowed rows struck out; the store's dict / callable matching rules; RowSet validation; rarc_search_rows / rarc_strike_rows
argument checks."""
import ctypes

import numpy as np
import pytest

from tests import l2_ref, subset_ref


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _corpus(rng, n, d):
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[10:20] = X[3]                      # rows 10..19 are copies of row 3: ties, decided by id
    X[40] = 0.0                          # a zero row: score +0.0 / -0.0 territory
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q[1] = X[3]
    return X, Q


@pytest.mark.parametrize("storage", ["f16", "f32"])
@pytest.mark.parametrize("normalize", [True, False])
def test_restatement_is_the_full_ranking_struck_and_cut(oracle, storage, normalize):
    rng = np.random.default_rng(11)
    n, d = 300, 72
    X, Q = _corpus(rng, n, d)
    rows = l2_ref.stored_rows(oracle, X, storage, normalize)
    qp = subset_ref.prepared_queries(oracle, Q, rows.shape[1], normalize)
    if storage == "f16":
        I_full, D_full, _ = oracle.flat_search_f16(rows, qp, n, id_base=5)
    else:
        I_full, D_full, _ = oracle.flat_search_f32(rows, qp, n, id_base=5)
    for allowed in (np.array([3, 11, 12, 17, 19, 40, 250]), np.sort(rng.choice(n, 150, replace=False)), np.arange(n),
                    np.array([7]), np.zeros(0, np.int64)):
        for k in (1, 5, 200):
            D, I = subset_ref.search(oracle, rows, Q, k, allowed, "ip", normalize, id_base=5)
            rD, rI = subset_ref.strike(D_full, I_full, allowed, k, id_base=5)
            assert np.array_equal(I, rI) and np.array_equal(_bits(D), _bits(rD)), (storage, normalize, allowed.size, k)
    # the copies of row 3 that are allowed come out together, by id
    D, I = subset_ref.search(oracle, rows, Q, 3, np.array([3, 11, 12, 17, 19, 40, 250]), "ip", normalize)
    assert I[1, :3].tolist() == [3, 11, 12] and D[1, 0] == D[1, 2]


@pytest.mark.parametrize("storage", ["f16", "f32"])
def test_l2_restatement_is_the_full_ranking_struck_and_cut(oracle, storage):
    rng = np.random.default_rng(12)
    n, d = 200, 40
    X, Q = _corpus(rng, n, d)
    rows = l2_ref.stored_rows(oracle, X, storage, False)
    D_full, I_full = l2_ref.search(oracle, X, Q, n, storage, rows=rows)
    for allowed in (np.array([3, 11, 12, 17, 40, 150]), np.sort(rng.choice(n, 90, replace=False)), np.zeros(0, np.int64)):
        for k in (1, 4, 120):
            D, I = subset_ref.search(oracle, rows, Q, k, allowed, "l2")
            rD, rI = subset_ref.strike(D_full, I_full, allowed, k, l2=True)
            assert np.array_equal(I, rI) and np.array_equal(_bits(D), _bits(rD)), (storage, allowed.size, k)
    D, I = subset_ref.search(oracle, rows, Q, 3, np.array([3, 11, 12, 17, 40, 150]), "l2")
    assert I[1, :3].tolist() == [3, 11, 12]


def test_ordkey_ranks_plus_zero_above_minus_zero():
    k = subset_ref.ordkey(np.array([1.0, 0.0, -0.0, -1.0, np.inf, -np.inf], np.float32)).astype(np.int64)
    assert k[4] > k[0] > k[1] > k[2] > k[3] > k[5]


def test_filter_matching_rules():
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import matching_rows, metadata_matches

    md = {"tenant": "a", "year": 2021, "tags": None}
    assert metadata_matches(md, {"tenant": "a"}) and not metadata_matches(md, {"tenant": "b"})
    assert metadata_matches(md, {"tenant": "a", "year": 2021}) and not metadata_matches(md, {"tenant": "a", "year": 2020})   # every key
    assert metadata_matches(md, {"year": [2020, 2021]}) and metadata_matches(md, {"year": (2021,)})                         # membership
    assert not metadata_matches(md, {"year": [2019]}) and not metadata_matches(md, {"year": []})
    assert not metadata_matches(md, {"file": "x"}) and not metadata_matches({}, {"tenant": "a"})                              # missing key
    assert metadata_matches(md, {"tags": None}) and metadata_matches(md, {})
    assert metadata_matches(md, lambda m: m["year"] > 2020) and not metadata_matches(md, lambda m: m.get("tenant") == "b")
    with pytest.raises(ValueError):
        metadata_matches(md, "tenant=a")
    mds = [{"tenant": "a"}, {"tenant": "b"}, None, {"tenant": "a", "year": 1}]
    assert matching_rows(mds, {"tenant": "a"}).tolist() == [0, 3] and matching_rows(mds, lambda m: not m).tolist() == [2]
    assert matching_rows(mds, {"tenant": "c"}).dtype == np.int64 and matching_rows(mds, {"tenant": "c"}).size == 0


def test_rowset_validation():
    from rag_arc_amd.hip.engine import RowSet

    assert RowSet.sorted_rows([9, 2, 2, 7], 10).tolist() == [2, 7, 9]
    assert RowSet.sorted_rows(np.array([False, True, True, False]), 4).tolist() == [1, 2]
    assert RowSet.sorted_rows([], 4).size == 0 and RowSet.sorted_rows(np.zeros(0, np.int64), 0).size == 0
    import torch

    assert RowSet.sorted_rows(torch.tensor([3, 1]), 4).tolist() == [1, 3]
    for bad, n in (([10], 10), ([-1], 10), ([0, 4], 4), (np.array([True, False]), 3), ([0.5], 4), (np.array([7], np.uint64), 7)):
        with pytest.raises(ValueError):
            RowSet.sorted_rows(bad, n)


def test_search_rows_validates_its_arguments_without_a_gpu():
    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    p = ctypes.c_void_p(256)
    good = dict(rows=p, fmt=0, n=100, d_pad=128, qb=p, nq=1, lst=p, m=10, k=5, base=0, xn=None, l2=0, oi=p, os=p, st=p, ws=p, wsb=1 << 30)

    def call(**kw):
        a = {**good, **kw}
        return lib.rarc_search_rows(a["rows"], a["fmt"], a["n"], a["d_pad"], a["qb"], a["nq"], a["lst"], a["m"], a["k"], a["base"],
                                    a["xn"], a["l2"], a["oi"], a["os"], a["st"], a["ws"], a["wsb"], None)

    for null in ("rows", "qb", "lst", "oi", "os", "st", "ws"):
        assert call(**{null: None}) == -1 and b"null pointer" in lib.rarc_last_error(), null
    assert call(k=0) == -1 and call(k=8193) == -1 and call(nq=0) == -1 and call(nq=257) == -1
    assert call(d_pad=100) == -4 and call(d_pad=4224) == -4 and call(d_pad=0) == -4
    assert call(fmt=1) == -1 and call(fmt=3) == -1 and b"fmt" in lib.rarc_last_error()
    assert call(l2=1) == -1 and b"d_xn" in lib.rarc_last_error()
    assert call(m=-1) == -1 and call(m=101) == -1
    assert call(wsb=1024) == -3                                         # workspace too small
    assert lib.rarc_search_rows_workspace_bytes(0, 5) == 0 and lib.rarc_search_rows_workspace_bytes(1, 8193) == 0
    # bounded whatever m is: k + one slab of keys per query
    assert lib.rarc_search_rows_workspace_bytes(256, 8192) <= 256 * (8192 + 32768) * 8 + 2048
    assert lib.rarc_search_rows_workspace_bytes(1, 10) <= (10 + 262144) * 8 + 2048
    assert lib.rarc_strike_rows(None, p, 1, 10, p, 100, 0, 5, 0, p, p, p, None) == -1
    assert lib.rarc_strike_rows(p, p, 1, 10, p, 100, 0, 0, 0, p, p, p, None) == -1
