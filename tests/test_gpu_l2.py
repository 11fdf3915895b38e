"""Metric "l2": exact squared-Euclidean top-k (faiss.IndexFlatL2; VectorStore_Faiss.py:73-146) on the chunked-GEMM path
(csrc/wide.hip, rarc_search_wide_l2; csrc/l2.hip, rarc_row_sqnorms).

Parity: ids AND distance bits against the CPU restatement (tests/l2_ref.py: dist = max(0, (qn + xn) - 2 ip) of three
canonical fp32 inner products, (dist asc, id asc)) for every query of every case — fp16 and fp32 rows, d from 64 to 3072,
n from a few hundred to 200k (ragged), k from 1 to 5000 and beyond n, id_base != 0, rows with norms over 0.1 .. 10 (where the
L2 answer must differ from the inner-product answer), exact duplicates, a query bit-equal to a stored row, 40,000
near-duplicates (the candidate lists overflow and the search repeats), normalize=True, the xn array through the index's
life, the store and its retriever modes, and the refusals."""
import numpy as np
import pytest

from tests import l2_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from rag_arc_amd.hip import engine

    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(D, I, ref_D, ref_I):
    return np.array_equal(I, ref_I) and np.array_equal(_bits(D), _bits(ref_D))


def _spread(rng, n, d, nq=5):
    """Rows and queries with norms log-uniform over 0.1 .. 10; two exact duplicates of row 5; query 0 = stored row 17."""
    X = rng.standard_normal((n, d)).astype(np.float32)
    X *= (10.0 ** rng.uniform(-1, 1, (n, 1)) / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q *= (10.0 ** rng.uniform(-1, 1, (nq, 1)) / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    if n > 40:
        X[n // 2] = X[5]
        X[n - 1] = X[5]
        Q[1] = X[5] * np.float32(1.0009765625)
        X[17] = X[17].astype(np.float16).astype(np.float32)      # representable in either storage: the stored row IS this row
        Q[0] = X[17]
    return X, Q


CASES = [
    # storage, d, n, k, id_base
    ("f16", 64, 300, 1, 0),
    ("f16", 64, 300, 400, 7),             # k > n
    ("f16", 384, 5_003, 10, 0),
    ("f16", 768, 200_003, 100, 1_000_000),
    ("f16", 1030, 70_001, 1000, 0),
    ("f16", 1536, 120_077, 5000, 0),
    ("f16", 3072, 40_009, 10, 3),
    ("f32", 64, 777, 10, 0),
    ("f32", 384, 20_011, 5000, 0),
    ("f32", 768, 100_003, 1000, 11),
    ("f32", 1536, 30_001, 100, 0),
    ("f32", 3072, 9_001, 1, 0),
    ("f32", 1030, 650, 700, 0),           # k > n
]


@pytest.mark.parametrize("storage,d,n,k,id_base", CASES)
def test_l2_matches_the_restatement(hip, oracle, storage, d, n, k, id_base):
    rng = np.random.default_rng(d * 7 + n + k)
    X, Q = _spread(rng, n, d)
    idx = hip.FlatIndexF16(d, metric="l2", storage=storage, id_base=id_base)
    assert idx.wide and not idx.normalize
    for s0 in range(0, n, 70_000):
        idx.add(X[s0:s0 + 70_000])
    D, I = idx.search(Q, k)
    ref_D, ref_I = l2_ref.search(oracle, X, Q, k, storage, id_base=id_base)
    assert _same(D, I, ref_D, ref_I), (storage, d, n, k)
    kk = min(k, n)
    assert (np.diff(D[:, :kk], axis=1) >= 0).all()                               # ascending
    assert (I[:, kk:] == -1).all() and np.isposinf(D[:, kk:]).all()              # beyond the stored rows
    assert I[0, 0] == id_base + 17 and D[0, 0] == 0.0 and not np.signbit(D[0, 0])    # the query that is a stored row
    if kk >= 3:                                                                  # the three copies of row 5, by id
        pos = [int(np.nonzero(I[1] == id_base + r)[0][0]) for r in (5, n // 2, n - 1)]
        assert pos[0] + 1 == pos[1] and pos[1] + 1 == pos[2] and D[1, pos[0]] == D[1, pos[2]]
    # with norms over two decades the nearest rows are not the rows of largest inner product: the case shows something
    ip_I = l2_ref.ip_topk(oracle, X, Q, kk, storage) + id_base
    if kk < n:
        assert any(set(I[q, :kk].tolist()) != set(ip_I[q].tolist()) for q in range(Q.shape[0]))
    else:
        assert not np.array_equal(I[:, :kk], ip_I)
    handle = idx.search_async(Q, k)
    Dh, Ih = handle.host()
    assert _same(Dh, Ih, D, I)
    # xn is the canonical |row|^2 of the stored rows, bit for bit
    rows = l2_ref.stored_rows(oracle, X, storage)
    xn = l2_ref.sqnorms_f16(rows) if storage == "f16" else l2_ref.canon_dot(rows, rows)
    assert np.array_equal(_bits(idx.row_sqnorms.cpu().numpy()), _bits(xn))


def test_256_queries_and_more(hip, oracle):
    """A full query block and a batch of several blocks."""
    rng = np.random.default_rng(256)
    X, Q = _spread(rng, 30_011, 256, nq=300)
    idx = hip.FlatIndexF16(256, metric="l2")
    idx.add(X)
    D, I = idx.search(Q, 20)
    assert _same(D, I, *l2_ref.search(oracle, X, Q, 20))


def test_near_duplicates_overflow_and_repeat(hip, oracle):
    """40,000 near-duplicates of one row (+ 8,000 others): every one of them lies inside the error margin of the k-th
    smallest distance of a query on that row, the candidate lists fill up, and the search is answered again with more room."""
    rng = np.random.default_rng(40)
    d, k = 768, 300
    base = rng.standard_normal((1, d)).astype(np.float32)
    dup = np.repeat(base, 40_000, axis=0)
    dup[::3] += (rng.standard_normal((len(dup[::3]), d)) * 1e-4).astype(np.float32)
    X = np.concatenate([dup, rng.standard_normal((8_000, d)).astype(np.float32) * 2.0])
    rng.shuffle(X)
    Q = np.concatenate([base, base * np.float32(1.25), rng.standard_normal((3, d)).astype(np.float32)])
    idx = hip.FlatIndexF16(d, metric="l2")
    idx.add(X)
    D, I = idx.search(Q, k)
    first_cap = ((max(16384, 2 * k) + 255) // 256) * 256 + 256
    assert idx.last_wide_cap > first_cap                       # the repeat happened
    assert _same(D, I, *l2_ref.search(oracle, X, Q, k))


@pytest.mark.parametrize("storage,d,n,k", [("f16", 384, 50_021, 100), ("f32", 1536, 20_003, 1000), ("f16", 64, 500, 10)])
def test_normalize_L2(hip, oracle, storage, d, n, k):
    """normalize=True (the reference's normalize_L2 + IndexFlatL2): both sides normalised as for cosine, distances equal the
    restatement, and the ids equal the cosine answer's wherever the cosine gaps exceed B.
    B: dist / 2 = (qn + xn)/2 - ip up to the two roundings of dist (<= 2^-23 * 4 * 1.01 in all), so two rows whose cosines
    differ by more than |xn_i - 1|/2 + |xn_j - 1|/2 + 2^-21 are ordered alike: B = max_j |xn_j - 1| + 2^-21.
    So that the comparison covers every query, each one gets a ladder of 20 planted rows at cosines 0.98, 0.96 .. 0.60 (steps of
    0.02; B < 0.01: a unit row rounded to fp16 has |xn - 1| <= 2 * 2^-11 + ...), far above the random rows' cosines (< 0.6):
    the first min(k, 19) ranks of every query are then settled by construction, and the test asserts that they are."""
    rng = np.random.default_rng(n)
    X, Q = _spread(rng, n, d)
    Q[1] = rng.standard_normal(d).astype(np.float32)            # (no query on the duplicate rows here: their gaps are 0)
    spots = rng.choice(np.arange(40, n // 2), size=(Q.shape[0], 20), replace=False)
    for qi in range(Q.shape[0]):
        qh = Q[qi].astype(np.float64) / np.linalg.norm(Q[qi].astype(np.float64))
        for j in range(20):
            c = 0.98 - 0.02 * j
            r = rng.standard_normal(d)
            r -= (r @ qh) * qh
            r /= np.linalg.norm(r)
            X[spots[qi, j]] = ((c * qh + np.sqrt(1 - c * c) * r) * 10.0 ** rng.uniform(-1, 1)).astype(np.float32)
    idx = hip.FlatIndexF16(d, metric="l2", storage=storage, normalize=True)
    idx.add(X)
    D, I = idx.search(Q, k)
    assert _same(D, I, *l2_ref.search(oracle, X, Q, k, storage, normalize=True))
    cos = hip.FlatIndexF16(d, metric="cosine", storage=storage)
    cos.add(X)
    Dc, Ic = cos.search(Q, k + 1)
    xn = idx.row_sqnorms.cpu().numpy().astype(np.float64)
    B = float(np.abs(xn - 1).max()) + 2.0 ** -21
    gaps = -np.diff(Dc.astype(np.float64), axis=1)                                # [nq][k], gap between ranks p and p + 1
    clear = gaps > B
    settled = clear[:, 1:] & clear[:, :-1]                                        # ranks 1 .. k-1: both neighbours far
    settled = np.concatenate([clear[:, :1], settled], axis=1)                     # rank 0: the one below
    m = min(k, 19)
    assert B < 0.01 and settled[:, :m].all()                                      # the planted ladders: every query is covered
    assert np.array_equal(I[settled], Ic[:, :k][settled])
    assert np.array_equal(I[:, :m], Ic[:, :m])


def test_xn_follows_the_index_through_its_life(hip, oracle, tmp_path):
    """add in uneven pieces, remove_rows, save / load, reset + add: after each step the answer equals the restatement on the
    surviving rows and xn equals a fresh recomputation, bit for bit."""
    rng = np.random.default_rng(77)
    d, k = 384, 50
    X, Q = _spread(rng, 9_000, d)

    def check(idx, live):
        rows = l2_ref.stored_rows(oracle, live)
        assert idx.ntotal == len(live)
        assert np.array_equal(idx.rows.cpu().numpy().view(np.uint16), rows)
        assert np.array_equal(_bits(idx.row_sqnorms.cpu().numpy()), _bits(l2_ref.sqnorms_f16(rows)))
        D, I = idx.search(Q, k)
        assert _same(D, I, *l2_ref.search(oracle, live, Q, k, rows=rows))

    idx = hip.FlatIndexF16(d, metric="l2")
    at = 0
    for piece in (1, 31, 1000, 33, 4097, 9_000 - 5162):                        # 1. uneven pieces
        idx.add(X[at:at + piece])
        at += piece
        check(idx, X[:at])
    holes = np.unique(np.concatenate([rng.integers(0, 9_000, 700), [0, 17, 8_999]]))
    assert idx.remove_rows(holes) == len(holes)                                # 2. remove_rows
    live = np.delete(X, holes, axis=0)
    check(idx, live)
    path = str(tmp_path / "l2.rarc")
    idx.save_shard(path)                                                       # 3. save / load
    again = hip.FlatIndexF16(d, metric="l2")
    again.load_shard(path)
    check(again, live)
    again.add(X[:100])
    check(again, np.concatenate([live, X[:100]]))
    idx.reset()                                                                # 4. reset, then add again
    assert idx.ntotal == 0
    De, Ie = idx.search(Q, 3)
    assert (Ie == -1).all() and np.isposinf(De).all()
    idx.add(X[4000:4500])
    check(idx, X[4000:4500])
    import torch
    fresh = hip.FlatIndexF16(d, metric="l2", growable=False)                   # adopted rows (no copy) and a plain buffer
    fresh.add_rows_f16(torch.from_numpy(l2_ref.stored_rows(oracle, X[:6400]).view(np.float16)).cuda(), 10.1)
    check(fresh, X[:6400])
    fresh.add(X[6400:7000])
    check(fresh, X[:7000])


def test_store_and_retriever_modes(hip, oracle, tmp_path):
    """HipFlatVectorStore(metric="l2") and its config through similarity, similarity_score_threshold and mmr; delete and
    save_local / load_local; relevance = _euclidean_relevance_score_fn(dist)."""
    from rag_arc_amd.config.modules import HipFlatVectorStoreConfig
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from rag_arc_amd.encapsulation.database.vector_db.base import VectorStore
    from tests.helpers import HashEmbeddings

    import typing

    assert "l2" in typing.get_args(typing.get_type_hints(HipFlatVectorStoreConfig)["metric"])
    emb = HashEmbeddings(384)
    texts = [f"l2 document {i}" for i in range(2500)]
    ids = [f"e{i}" for i in range(2500)]
    X = np.asarray(emb.embed_documents(texts), dtype=np.float32)
    for normalize in (False, True):
        store = HipFlatVectorStore(emb, metric="l2", normalize_L2=normalize)
        assert store._select_relevance_score_fn() is store._euclidean_relevance_score_fn
        for s0 in (0, 700, 701, 2000):
            e0 = {0: 700, 700: 701, 701: 2000, 2000: 2500}[s0]
            store.add_texts(texts[s0:e0], ids=ids[s0:e0])
        assert store.index.metric == "l2" and store.index.normalize == normalize
        query = "l2 document 1234 and then some"
        qv = np.asarray([emb.embed_query(query)], dtype=np.float32)
        ref_D, ref_I = l2_ref.search(oracle, X, qv, 8, normalize=normalize)
        got = store.similarity_search_with_score(query, k=8)
        assert [d.id for d, _ in got] == [ids[i] for i in ref_I[0]]
        assert np.array_equal(_bits([s for _, s in got]), _bits(ref_D[0]))
        assert [s for _, s in got] == sorted(s for _, s in got)                                      # nearest first
        assert store.similarity_search_with_score(texts[99], k=1)[0][0].id == "e99"
        rel = store.similarity_search_with_relevance_scores(query, k=8)
        assert [r for _, r in rel] == [VectorStore._euclidean_relevance_score_fn(float(s)) for _, s in got]
        batch = store.batch_similarity_search_with_score([query, texts[5]], k=8)
        assert [(d.id, s) for d, s in batch[0]] == [(d.id, s) for d, s in got] and batch[1][0][0].id == "e5"
        # the retriever modes
        sim = store.as_retriever(search_type="similarity", search_kwargs={"k": 8}).invoke(query)
        assert [d.id for d in sim] == [d.id for d, _ in got]
        if normalize:             # (relevance 1 - dist / sqrt 2 reaches [0, 1] only for near rows: the text itself, dist 0)
            kept = store.as_retriever(search_type="similarity_score_threshold",
                                      search_kwargs={"k": 8, "score_threshold": 0.5}).invoke(texts[77])
            rel77 = store.similarity_search_with_relevance_scores(texts[77], k=8)
            assert [d.id for d in kept] == ["e77"] and abs(rel77[0][1] - 1.0) < 1e-3 and all(r < 0.5 for _, r in rel77[1:])
        mmr = store.as_retriever(search_type="mmr", search_kwargs={"k": 4, "fetch_k": 12}).invoke(query)
        fetched = [d.id for d, _ in store.similarity_search_with_score(query, k=12)]
        assert len(mmr) == 4 and mmr[0].id == fetched[0] and all(d.id in fetched for d in mmr)
        # delete (compaction: xn recomputed from the first hole), save_local / load_local
        assert store.delete(["e1234", "e0", ids[int(ref_I[0][0])]]) is True
        gone = sorted({1234, 0, int(ref_I[0][0])})
        live = np.delete(X, gone, axis=0)
        live_ids = [i for j, i in enumerate(ids) if j not in gone]
        ref_D2, ref_I2 = l2_ref.search(oracle, live, qv, 8, normalize=normalize)
        got2 = store.similarity_search_with_score(query, k=8)
        assert [d.id for d, _ in got2] == [live_ids[i] for i in ref_I2[0]]
        assert np.array_equal(_bits([s for _, s in got2]), _bits(ref_D2[0]))
        store.save_local(str(tmp_path / f"l2_{normalize}"))
        again = HipFlatVectorStore.load_local(str(tmp_path / f"l2_{normalize}"), emb)
        assert again.metric == "l2" and again.normalize_L2 == normalize and again.index.metric == "l2"
        assert [(d.id, s) for d, s in again.similarity_search_with_score(query, k=8)] == [(d.id, s) for d, s in got2]
        rows = l2_ref.stored_rows(oracle, live, normalize=normalize)
        assert np.array_equal(_bits(again.index.row_sqnorms.cpu().numpy()), _bits(l2_ref.sqnorms_f16(rows)))
        assert store.delete(None) is True and store.similarity_search(query, k=3) == []
    # cosine and ip stores are what they were
    ip = HipFlatVectorStore.from_texts(texts[:500], emb, ids=ids[:500], metric="ip")
    assert ip.index.metric == "ip" and not ip.index.normalize and ip.index.row_sqnorms is None
    assert HipFlatVectorStore(emb, metric="ip", normalize_L2=True)._engine_metric() == "cosine"


def test_refusals_come_before_any_launch():
    """fp8 rows, the int8 shadow image and the sharded index / store do not answer metric "l2": RarcUnsupported at
    construction, the message naming what does."""
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import HipShardedFlatVectorStore
    from rag_arc_amd.hip import binding as B
    from rag_arc_amd.hip.engine import FlatIndexF16
    from rag_arc_amd.hip.sharded import ShardedFlatSearch
    from tests.helpers import HashEmbeddings

    with pytest.raises(B.RarcUnsupported, match="'f16' or 'f32'"):
        FlatIndexF16(256, metric="l2", storage="f8")
    with pytest.raises(B.RarcUnsupported, match="shadow"):
        FlatIndexF16(256, metric="l2", shadow=True)
    with pytest.raises(B.RarcUnsupported, match="scan='auto'"):
        FlatIndexF16(256, metric="l2", scan="q8")
    with pytest.raises(B.RarcUnsupported):
        FlatIndexF16(4200, metric="l2")
    with pytest.raises(B.RarcUnsupported, match="'f16' or 'f32'"):
        HipFlatVectorStore(HashEmbeddings(64), metric="l2", storage="f8")
    with pytest.raises(B.RarcUnsupported, match="HipFlatVectorStore"):
        HipShardedFlatVectorStore(HashEmbeddings(64), metric="l2")
    idx = FlatIndexF16(64, metric="l2")
    with pytest.raises(B.RarcUnsupported, match="one FlatIndexF16"):
        ShardedFlatSearch(idx)
    idx.add(np.ones((40, 64), np.float32))
    with pytest.raises(B.RarcUnsupported, match="8192"):
        idx.search(np.ones((1, 64), np.float32), 9000)
    with pytest.raises(ValueError):
        FlatIndexF16(64, metric="cosine", normalize=False)


def test_scores_beyond_the_fp16_range_are_refused_and_just_under_it_answered(hip, oracle):
    """Without normalisation the first chunk's fp16 scores must stay finite: |q| * max |row| * 1.01 >= 2^15 is refused before
    the first kernel of the search (the power-of-two query scaling of metric "ip" is not linear in a distance); just under
    the limit the answer is the restatement's, bit for bit."""
    import torch

    rng = np.random.default_rng(15)
    n, d, k = 3_000, 128, 25
    X = rng.standard_normal((n, d)).astype(np.float32)
    X *= (rng.uniform(20, 100, (n, 1)) / np.linalg.norm(X, axis=1, keepdims=True)).astype(np.float32)
    X[77] *= np.float32(100.0 / np.linalg.norm(X[77]))                           # max |row| = 100
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q *= (290.0 / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)     # 290 * 100 * 1.01 = 29,290 < 32,768
    Q[3] = X[77] * np.float32(2.9)
    idx = hip.FlatIndexF16(d, metric="l2")
    idx.add(X)
    D, I = idx.search(Q, k)
    ref_D, ref_I = l2_ref.search(oracle, X, Q, k)
    assert _same(D, I, ref_D, ref_I) and np.isfinite(D).all() and float(D.max()) > 65504.0
    big = Q * np.float32(330.0 / 290.0)                                          # 330 * 100 * 1.01 = 33,330 >= 32,768
    torch.cuda.synchronize()
    with pytest.raises(hip.B.RarcUnsupported, match="fp16 range"):
        idx.search(big, k)
    with pytest.raises(hip.B.RarcUnsupported, match="fp16 range"):
        idx.search_async(big, k)
    D2, I2 = idx.search(Q, k)                                                    # the index answers as before
    assert _same(D2, I2, ref_D, ref_I)
    nrm = hip.FlatIndexF16(d, metric="l2", normalize=True)                       # normalised: any scale goes in
    nrm.add(X)
    Dn, In = nrm.search(big, k)
    assert _same(Dn, In, *l2_ref.search(oracle, X, big, k, normalize=True))


def test_score_threshold_on_an_unnormalised_store(hip, oracle):
    """similarity_score_threshold with metric "l2" and no normalisation: relevance = 1 - dist / sqrt 2 lies in [0, 1] for
    embeddings of small norm; a threshold between the 3rd and 4th best relevance of the restatement keeps exactly its 3
    nearest rows, nearest first."""
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from rag_arc_amd.encapsulation.database.vector_db.base import VectorStore
    from tests.helpers import HashEmbeddings

    class SmallEmbeddings(HashEmbeddings):
        def _one(self, text):
            return (super()._one(text) * np.float32(0.02)).astype(np.float32)     # |v| ~ 0.02 sqrt(384) = 0.39

    emb = SmallEmbeddings(384)
    texts = [f"small document {i}" for i in range(600)]
    ids = [f"s{i}" for i in range(600)]
    X = np.asarray(emb.embed_documents(texts), dtype=np.float32)
    store = HipFlatVectorStore.from_texts(texts, emb, ids=ids, metric="l2")
    assert store.index.metric == "l2" and not store.index.normalize
    query = "a question about small documents"
    qv = np.asarray([emb.embed_query(query)], dtype=np.float32)
    ref_D, ref_I = l2_ref.search(oracle, X, qv, 8)
    rel = [VectorStore._euclidean_relevance_score_fn(float(v)) for v in ref_D[0]]
    assert all(0.0 <= r <= 1.0 for r in rel) and rel[2] > rel[3]
    thr = (rel[2] + rel[3]) / 2
    got = store.similarity_search_with_relevance_scores(query, k=8, score_threshold=thr)
    assert [d.id for d, _ in got] == [ids[i] for i in ref_I[0][:3]] and [r for _, r in got] == rel[:3]
    kept = store.as_retriever(search_type="similarity_score_threshold",
                              search_kwargs={"k": 8, "score_threshold": thr}).invoke(query)
    assert [d.id for d in kept] == [ids[i] for i in ref_I[0][:3]]
    everything = store.as_retriever(search_type="similarity_score_threshold",
                                    search_kwargs={"k": 8, "score_threshold": 0.0}).invoke(query)
    assert [d.id for d in everything] == [ids[i] for i in ref_I[0]]


def test_c_abi_checks_its_arguments(hip):
    import ctypes

    lib = hip.B.load_library()
    p = ctypes.c_void_p(256)
    assert lib.rarc_row_sqnorms(None, 0, 10, 128, 0, p, None) == -1 and b"null pointer" in lib.rarc_last_error()
    assert lib.rarc_row_sqnorms(p, 1, 10, 128, 0, p, None) == -1 and b"fmt" in lib.rarc_last_error()
    assert lib.rarc_row_sqnorms(p, 0, 10, 100, 0, p, None) != 0 and b"padded dim" in lib.rarc_last_error()
    assert lib.rarc_row_sqnorms(p, 0, 10, 128, 11, p, None) == -1 and b"first_row" in lib.rarc_last_error()
    assert lib.rarc_search_wide_l2(p, None, 0, 10, 128, 1.0, 0.0, None, p, 1, 1, 0, p, p, p, p, 1 << 30, 16640, None) == -1
    assert b"d_xn" in lib.rarc_last_error()
    assert lib.rarc_search_wide_l2(p, None, 0, 10, 128, 1.0, 0.0, p, p, 1, 9000, 0, p, p, p, p, 1 << 30, 16640, None) == -1
