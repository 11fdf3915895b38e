"""Filtered search on the GPU: FlatIndexF16.search_filtered (csrc/subset.hip: rarc_search_rows, rarc_strike_rows) and the
stores' `filter=`.  Ids AND score bits against the CPU restatement tests/subset_ref.py — the canonical scores of the allowed
rows, (score desc, id asc) / metric "l2" (dist asc, id asc), cut at k — for every query of every case, under each forced
strategy and "auto".  n = 5000 rows; rows 10..19 are copies of row 3, some of them allowed and some not, and query 0 IS row 3:
the id tie-break and the striking both show at the top of its answer."""
import asyncio

import numpy as np
import pytest

from tests import l2_ref, subset_ref
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu

N = 5000
_IN, _OUT = [3, 11, 12, 17], [10, 13]         # copies of row 3 that are allowed / struck whenever the set has room for them


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


_DATA: dict = {}


def _data(d, nq):
    """Rows and queries of one dimension, made once and left unchanged."""
    if (d, nq) not in _DATA:
        rng = np.random.default_rng(1000 + d)
        X = rng.standard_normal((N, d)).astype(np.float32)
        X[10:20] = X[3]
        Q = np.random.default_rng(d + nq).standard_normal((nq, d)).astype(np.float32)
        Q[0] = X[3]
        _DATA[(d, nq)] = (X, Q)
    return _DATA[(d, nq)]


def _allowed(kind, k, seed=0):
    rng = np.random.default_rng(seed + 77)
    others = np.setdiff1d(np.arange(N), np.array(_IN + _OUT))
    m = {"zero": 0, "one": 1, "k-1": k - 1, "k": k, "1%": N // 100, "50%": N // 2, "all": N}[kind]
    if m == N:
        return np.arange(N)
    if m <= 1:
        return np.array([12][:m], dtype=np.int64)
    forced = np.array(_IN[: min(m, len(_IN))])
    return np.sort(np.concatenate([forced, rng.choice(others, m - forced.size, replace=False)])).astype(np.int64)


def _index(hip, X, storage, metric):
    idx = hip.FlatIndexF16(X.shape[1], metric=metric, storage=storage)
    idx.add(X)
    return idx


CASES = [
    # storage, metric, d, nq, k, allowed rows
    ("f16", "cosine", 64, 1, 1, "zero"),
    ("f16", "cosine", 64, 3, 10, "one"),
    ("f16", "ip", 200, 256, 10, "k-1"),
    ("f32", "cosine", 200, 3, 100, "k"),
    ("f16", "l2", 64, 300, 10, "1%"),
    ("f32", "ip", 1536, 3, 100, "50%"),
    ("f16", "cosine", 1536, 1, 1500, "all"),
    ("f32", "l2", 200, 3, 1500, "50%"),
    ("f16", "ip", 64, 300, 100, "50%"),
    ("f32", "cosine", 64, 256, 1, "1%"),
]


@pytest.mark.parametrize("storage,metric,d,nq,k,kind", CASES)
def test_filtered_search_matches_the_restatement(hip, oracle, storage, metric, d, nq, k, kind):
    X, Q = _data(d, nq)
    allowed = _allowed(kind, k)
    normalize = metric == "cosine"
    idx = _index(hip, X, storage, metric)
    rows = l2_ref.stored_rows(oracle, X, storage, normalize)
    ref_D, ref_I = subset_ref.search(oracle, rows, Q, k, allowed, "l2" if metric == "l2" else "ip", normalize)
    rs = idx.rowset(allowed)
    assert rs.m == allowed.size and len(rs) == allowed.size
    answers = {}
    for strategy in ("subset", "overfetch", "auto"):
        D, I = idx.search_filtered(Q, k, rs, strategy=strategy)
        assert D.shape == (nq, k) and I.shape == (nq, k)
        assert _same(D, I, ref_D, ref_I), (strategy, storage, metric, d, nq, k, kind)
        answers[strategy] = (D, I)
    assert _same(*answers["subset"], *answers["overfetch"])
    kk = min(k, allowed.size)
    assert (I[:, kk:] == -1).all() and (np.isposinf(D[:, kk:]) if metric == "l2" else np.isneginf(D[:, kk:])).all()
    assert np.isin(I[:, :kk], allowed).all()
    if allowed.size >= N // 100 and k >= 3:            # the allowed copies of row 3, by id, for the query that is row 3
        copies = [r for r in [3] + list(range(10, 20)) if r in set(allowed.tolist())]
        assert I[0, :3].tolist() == copies[:3] and _bits(D[0, 0]) == _bits(D[0, 2])
        assert kind == "all" or (copies[:3] == [3, 11, 12] and 10 not in I[0] and 13 not in I[0])     # struck rows stay out
    # a boolean mask and an unsorted list with duplicates make the same set
    mask = np.zeros(N, dtype=bool)
    mask[allowed] = True
    assert _same(*idx.search_filtered(Q[:2], k, idx.rowset(mask), strategy="subset"), ref_D[:2], ref_I[:2])
    shuffled = np.concatenate([allowed[::-1], allowed[:3]])
    assert _same(*idx.search_filtered(Q[:2], k, idx.rowset(shuffled), strategy="subset"), ref_D[:2], ref_I[:2])


def test_id_base_and_the_device_form(hip, oracle):
    X, Q = _data(64, 3)
    allowed = _allowed("1%", 10)
    idx = hip.FlatIndexF16(64, metric="cosine", id_base=1_000_000)
    idx.add(X)
    rows = l2_ref.stored_rows(oracle, X, "f16", True)
    ref_D, ref_I = subset_ref.search(oracle, rows, Q, 10, allowed, "ip", True, id_base=1_000_000)
    for strategy in ("subset", "overfetch"):
        ids, sc = idx.search_filtered_device(Q, 10, idx.rowset(allowed), strategy=strategy)
        assert ids.is_cuda and _same(sc.cpu().numpy(), ids.cpu().numpy(), ref_D, ref_I), strategy


def test_overfetch_falls_back_when_the_allowed_rows_rank_last(hip, oracle):
    """The allowed set is the 200 rows LEAST similar to the query: k' = 1.5 * 10 * 5000 / 200 + 32 = 407 results hold none of
    them, so "overfetch" hands the query to the row-list search — and the answer is still the reference's."""
    X, Q = _data(64, 3)
    rows = l2_ref.stored_rows(oracle, X, "f16", True)
    full_I = oracle.flat_search_f16(rows, oracle.normalize_L2(Q[:1]), N)[0]
    allowed = np.sort(full_I[0, -200:])
    idx = _index(hip, X, "f16", "cosine")
    rs = idx.rowset(allowed)
    before = dict(idx.filtered_stats)
    D, I = idx.search_filtered(Q[:1], 10, rs, strategy="overfetch")
    after = idx.filtered_stats
    assert after["fallback_queries"] == before["fallback_queries"] + 1
    assert after["overfetch_batches"] == before["overfetch_batches"] + 1 and after["subset_batches"] == before["subset_batches"]
    ref_D, ref_I = subset_ref.search(oracle, rows, Q[:1], 10, allowed, "ip", True)
    assert _same(D, I, ref_D, ref_I)
    assert I[0].tolist() == full_I[0, -200:-190].tolist()


def test_auto_takes_the_row_list_for_one_percent_and_over_fetch_for_half(hip, oracle):
    X, Q = _data(64, 256)
    idx = _index(hip, X, "f16", "cosine")
    rows = l2_ref.stored_rows(oracle, X, "f16", True)
    for kind, counter in (("1%", "subset_batches"), ("50%", "overfetch_batches")):
        allowed = _allowed(kind, 10)
        assert idx.filter_strategy(256, 10, allowed.size) == counter.split("_")[0]
        before = dict(idx.filtered_stats)
        D, I = idx.search_filtered(Q, 10, idx.rowset(allowed))
        after = idx.filtered_stats
        assert after[counter] == before[counter] + 1
        assert sum(after.values()) - sum(before.values()) == 1 + (after["fallback_queries"] - before["fallback_queries"])
        assert _same(D, I, *subset_ref.search(oracle, rows, Q, 10, allowed, "ip", True))


def test_a_stale_rowset_is_refused_and_a_fresh_one_answers(hip, oracle):
    from rag_arc_amd.hip.binding import RarcError

    X, Q = _data(64, 3)
    idx = _index(hip, X[:4000], "f16", "cosine")
    allowed = _allowed("1%", 10)
    allowed = allowed[allowed < 4000]
    rs = idx.rowset(allowed)
    idx.search_filtered(Q, 5, rs)
    idx.add(X[4000:])
    with pytest.raises(RarcError, match="changed"):
        idx.search_filtered(Q, 5, rs)
    rs = idx.rowset(allowed)
    holes = np.array([0, 11, 2500])
    idx.remove_rows(holes)
    with pytest.raises(RarcError, match="changed"):
        idx.search_filtered(Q, 5, rs, strategy="subset")
    kept = np.setdiff1d(np.arange(N), holes)
    Xc = X[kept]
    allowed_c = np.flatnonzero(np.isin(kept, allowed))           # the same documents under their new row numbers
    rows = l2_ref.stored_rows(oracle, Xc, "f16", True)
    ref = subset_ref.search(oracle, rows, Q, 5, allowed_c, "ip", True)
    for strategy in ("subset", "overfetch"):
        assert _same(*idx.search_filtered(Q, 5, idx.rowset(allowed_c), strategy=strategy), *ref)
    with pytest.raises(ValueError):
        idx.rowset([N])                                            # (N - 3 rows are left)
    other = _index(hip, X[:100], "f16", "cosine")
    with pytest.raises(ValueError):
        idx.search_filtered(Q, 5, other.rowset([1, 2]))


def test_the_empty_index_answers_padding(hip):
    idx = hip.FlatIndexF16(64, metric="l2")
    D, I = idx.search_filtered(np.zeros((2, 64), np.float32), 4, idx.rowset([]))
    assert (I == -1).all() and np.isposinf(D).all()


def test_engine_refusals(hip):
    from rag_arc_amd.hip.binding import RarcUnsupported

    X, Q = _data(64, 3)
    f8 = hip.FlatIndexF16(256, metric="cosine", storage="f8")
    with pytest.raises(RarcUnsupported, match="'f16' or 'f32'"):
        f8.rowset([0])
    sh = hip.FlatIndexF16(256, metric="cosine", shadow=True)
    with pytest.raises(RarcUnsupported, match="shadow"):
        sh.rowset([0])
    idx = _index(hip, X, "f16", "cosine")
    rs = idx.rowset([1, 2, 3])
    with pytest.raises(RarcUnsupported, match="twin"):
        idx.twin().search_filtered(Q, 2, rs)
    with pytest.raises(ValueError):
        idx.search_filtered(Q, 2, rs, strategy="fastest")
    with pytest.raises(ValueError):
        idx.search_filtered(Q, 0, rs)


# ------------------------------------------------------------------------------------------- the slab loop of rarc_search_rows
# 256 queries make a slab of 32768 listed rows (csrc/subset.hip: sub_slab_rows): m = 32768 is one slab exactly, 32769 one slab
# and one row, 70,001 three slabs — k keys carried from slab to slab through the select that only keeps them.  List positions
# 32767 and 32768, the two sides of the first slab edge, hold bit-identical rows in the list of 32769 (rows A[32767], A[32768])
# and in the list of every row (rows 32767, 32768); query 0 IS row 32767 and query 1 IS row A[32767], so the tie is at the top of
# an answer and the id has to decide it across the edge.
N_SLAB, D_SLAB, NQ_SLAB, EDGE = 70_001, 64, 256, 32768
_SLAB: dict = {}


def _slab_data():
    """Rows, queries and the three row lists; made once, left unchanged."""
    if not _SLAB:
        rng = np.random.default_rng(4242)
        X = rng.standard_normal((N_SLAB, D_SLAB)).astype(np.float32)
        others = np.setdiff1d(np.arange(N_SLAB), [EDGE - 1, EDGE])
        A = np.sort(rng.choice(others, EDGE + 1, replace=False)).astype(np.int64)
        X[EDGE] = X[EDGE - 1]
        X[A[EDGE]] = X[A[EDGE - 1]]
        Q = rng.standard_normal((NQ_SLAB, D_SLAB)).astype(np.float32)
        Q[0], Q[1] = X[EDGE - 1], X[A[EDGE - 1]]
        _SLAB.update(X=X, Q=Q, lists={EDGE: A[:EDGE], EDGE + 1: A, N_SLAB: np.arange(N_SLAB, dtype=np.int64)}, index={}, ref={})
    return _SLAB


def _slab_index(hip, storage, metric):
    S = _slab_data()
    if (storage, metric) not in S["index"]:
        idx = _index(hip, S["X"], storage, metric)
        S["index"][(storage, metric)] = (idx, {m: idx.rowset(a) for m, a in S["lists"].items()})
    return S["index"][(storage, metric)]


def _slab_reference(oracle, storage, metric, m, k):
    """subset_ref.search of the 256 queries over the list of m rows; computed once per list at the largest k asked of it (the
    answer for a smaller k is its prefix).  The restatement scores every row it is given, so it is given the listed rows alone,
    all of them allowed: position in the ascending list orders as the row number does, and the ids are mapped back."""
    S = _slab_data()
    key = (storage, metric, m)
    if key not in S["ref"] or S["ref"][key][0].shape[1] < k:
        normalize = metric == "cosine"
        a = S["lists"][m]
        rows = l2_ref.stored_rows(oracle, S["X"], storage, normalize)[a]
        Dr, Ir = subset_ref.search(oracle, rows, S["Q"], k, np.arange(a.size), "l2" if metric == "l2" else "ip", normalize)
        Ir = a[Ir]                                        # (k <= m: no padding)
        Dr.setflags(write=False)
        Ir.setflags(write=False)
        S["ref"][key] = (Dr, Ir)
    Dr, Ir = S["ref"][key]
    return Dr[:, :k], Ir[:, :k]


def _edge_tie_on_top(D, I, qi, lo, hi):
    return I[qi, :2].tolist() == [int(lo), int(hi)] and _bits(D[qi, 0]) == _bits(D[qi, 1])


@pytest.mark.parametrize("storage,metric", [("f16", "cosine"), ("f32", "l2")])
@pytest.mark.parametrize("m", [EDGE, EDGE + 1, N_SLAB])
def test_one_filter_slab_loop_matches_the_restatement(hip, oracle, storage, metric, m):
    S = _slab_data()
    idx, sets = _slab_index(hip, storage, metric)
    D, I = idx.search_filtered(S["Q"], 10, sets[m], strategy="subset")
    ref_D, ref_I = _slab_reference(oracle, storage, metric, m, 10)
    print(f"slab loop {storage} {metric} m={m}: ids equal {np.array_equal(I, ref_I)}, score bits equal "
          f"{np.array_equal(_bits(D), _bits(ref_D))}")
    assert _same(D, I, ref_D, ref_I), (storage, metric, m)
    A = S["lists"][EDGE + 1]
    if m == EDGE + 1:
        assert _edge_tie_on_top(D, I, 1, A[EDGE - 1], A[EDGE])
    if m == N_SLAB:
        assert _edge_tie_on_top(D, I, 0, EDGE - 1, EDGE) and _edge_tie_on_top(D, I, 1, A[EDGE - 1], A[EDGE])


def test_one_filter_slab_loop_at_the_largest_k(hip, oracle):
    """k = 8192 over three slabs: kept = k beside a full slab, the most keys the select ever holds."""
    S = _slab_data()
    idx, sets = _slab_index(hip, "f16", "cosine")
    D, I = idx.search_filtered(S["Q"], 8192, sets[N_SLAB], strategy="subset")
    ref_D, ref_I = _slab_reference(oracle, "f16", "cosine", N_SLAB, 8192)
    print(f"slab loop k=8192: ids equal {np.array_equal(I, ref_I)}, score bits equal {np.array_equal(_bits(D), _bits(ref_D))}")
    assert _same(D, I, ref_D, ref_I)
    assert _edge_tie_on_top(D, I, 0, EDGE - 1, EDGE)


@pytest.mark.parametrize("storage,metric", [("f16", "cosine"), ("f32", "l2")])
def test_the_grouped_form_answers_as_the_one_filter_form(hip, storage, metric):
    """csrc/subset.hip: "each query's answer is rarc_search_rows's for its list, bit for bit".  256 queries under one filter of
    32769 rows cross a slab edge; the first 40 of them, each carrying that filter, have a slab of 209 k rows and a single round."""
    S = _slab_data()
    idx, sets = _slab_index(hip, storage, metric)
    rs = sets[EDGE + 1]
    D_one, I_one = idx.search_filtered(S["Q"], 10, rs, strategy="subset")
    D_many, I_many = idx.search_filtered_many(S["Q"][:40], 10, [rs] * 40, strategy="subset")
    assert D_many.shape == (40, 10) and _same(D_many, I_many, D_one[:40], I_one[:40])
    A = S["lists"][EDGE + 1]
    assert _edge_tie_on_top(D_many, I_many, 1, A[EDGE - 1], A[EDGE])
    D_40, I_40 = idx.search_filtered(S["Q"][:40], 10, rs, strategy="subset")      # the one-filter form's single slab
    assert _same(D_40, I_40, D_many, I_many)


# ------------------------------------------------------------------------------------------------------------------ the store
def _store(embedding=None, **kw):
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore

    emb = embedding or HashEmbeddings(64)
    texts = [f"document {i}" for i in range(400)]
    metas = [{"tenant": "ab"[i % 2], "year": 2018 + i % 5} if i % 7 else {"year": 2018 + i % 5} for i in range(400)]
    store = HipFlatVectorStore(emb, metric="cosine", **kw)
    store.add_texts(texts, metas, ids=[f"id{i}" for i in range(400)])
    return store, texts, metas


def _expected(store, query, k, keep):
    """What the unfiltered call gives for the matching documents, in its order and with its scores, cut at k."""
    full = store.similarity_search_with_score(query, store.ntotal)
    return [(d, s) for d, s in full if keep(d.metadata)][:k]


FILTERS = [
    ({"tenant": "a"}, lambda m: m.get("tenant") == "a"),
    ({"tenant": "b", "year": [2019, 2021]}, lambda m: m.get("tenant") == "b" and m["year"] in (2019, 2021)),
    (lambda m: "tenant" not in m, lambda m: "tenant" not in m),
]


def test_dict_filter_returns_only_the_tenants_documents():
    store, _, _ = _store()
    got = store.similarity_search_with_score("document 5", 8, filter={"tenant": "a"})
    assert len(got) == 8 and all(d.metadata.get("tenant") == "a" for d, _ in got)
    want = _expected(store, "document 5", 8, lambda m: m.get("tenant") == "a")
    assert [(d.id, s) for d, s in got] == [(d.id, s) for d, s in want]


@pytest.mark.parametrize("which", range(len(FILTERS)))
def test_store_filters_through_every_entry_point(which):
    from rag_arc_amd.core.retrieval.dense import VectorStoreRetriever

    flt, keep = FILTERS[which]
    store, texts, _ = _store()
    q = "document 123"
    want = _expected(store, q, 6, keep)
    ids, scores = [d.id for d, _ in want], [s for _, s in want]
    assert len(want) == 6 and all(keep(d.metadata) for d, _ in want)
    handle = store.row_filter(flt)
    for f in (flt, handle):
        got = store.similarity_search_with_score(q, 6, filter=f)
        assert [d.id for d, _ in got] == ids and [s for _, s in got] == scores
        assert [d.id for d in store.similarity_search(q, 6, filter=f)] == ids
        vec = store.embedding.embed_query(q)
        assert [d.id for d in store.similarity_search_by_vector(vec, 6, filter=f)] == ids
        assert [(d.id, s) for d, s in store.similarity_search_by_vector_with_score(vec, 6, filter=f)] == list(zip(ids, scores))
        rel = store.similarity_search_with_relevance_scores(q, 6, filter=f)
        assert [d.id for d, _ in rel] == ids and [s for _, s in rel] == [1.0 - s for s in scores]
        batch = store.batch_similarity_search_with_score([q, "document 7"], 6, filter=f)
        assert [(d.id, s) for d, s in batch[0]] == list(zip(ids, scores))
        assert [d.id for d, _ in batch[1]] == [d.id for d, _ in _expected(store, "document 7", 6, keep)]
        assert [d.id for d in store.batch_similarity_search([q], 6, filter=f)[0]] == ids
        sc, rows = store.batch_search_by_vector(np.asarray([vec], np.float32), 6, filter=f)
        assert [f"id{r}" for r in rows[0]] == ids and sc[0].tolist() == scores
        got = asyncio.run(store.asimilarity_search_with_score(q, 6, filter=f))
        assert [(d.id, s) for d, s in got] == list(zip(ids, scores))
        assert [d.id for d in asyncio.run(store.asimilarity_search(q, 6, filter=f))] == ids
        retr = VectorStoreRetriever(store, search_kwargs={"k": 6, "filter": f})
        assert [d.id for d in retr.invoke(q)] == ids
        assert [d.id for d in retr.batch_invoke([q])[0]] == ids
    # fewer matches than k: what there is; no match: nothing
    n_match = sum(keep(d.metadata) for d in store._row_docs)
    assert len(store.similarity_search(q, 400, filter=flt)) == n_match
    assert store.similarity_search(q, 4, filter={"tenant": "nobody"}) == []
    # the handle goes stale with the rows
    from rag_arc_amd.hip.binding import RarcError

    store.delete(["id1"])
    with pytest.raises(RarcError, match="changed"):
        store.similarity_search(q, 6, filter=handle)
    assert [d.id for d in store.similarity_search(q, 6, filter=flt)] == [d.id for d, _ in _expected(store, q, 6, keep)]


def test_filter_over_a_columnar_docstore(hip):
    from rag_arc_amd.encapsulation.database.vector_db.docstore import ColumnarDocstore
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore

    emb = HashEmbeddings(64)
    texts = [f"document {i}" for i in range(300)]
    metas = [{"tenant": "ab"[i % 2], "year": 2018 + i % 5} for i in range(300)]
    idx = hip.FlatIndexF16(64, metric="cosine")
    idx.add(np.asarray(emb.embed_documents(texts), np.float32))
    store = HipFlatVectorStore(emb, metric="cosine").adopt(idx, ColumnarDocstore.from_texts(texts, [f"id{i}" for i in range(300)], metas))
    flt = {"tenant": "b", "year": (2020, 2022)}
    keep = lambda m: m["tenant"] == "b" and m["year"] in (2020, 2022)      # noqa: E731
    want = _expected(store, "document 9", 5, keep)
    got = store.similarity_search_with_score("document 9", 5, filter=flt)
    assert len(got) == 5 and [(d.id, s) for d, s in got] == [(d.id, s) for d, s in want]
    assert [d.id for d in store.similarity_search("document 9", 5, filter=store.row_filter(keep))] == [d.id for d, _ in want]
    bare = HipFlatVectorStore(emb, metric="cosine").adopt(idx, ColumnarDocstore.from_texts(texts))       # no metadata column
    assert bare.similarity_search("document 9", 5, filter=flt) == [] and len(bare.similarity_search("document 9", 5, filter={})) == 5


def test_store_refusals():
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore
    from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import HipShardedFlatVectorStore
    from rag_arc_amd.hip.binding import RarcUnsupported

    store, _, _ = _store()
    for call in (lambda: store.max_marginal_relevance_search("document 1", 3, filter={"tenant": "a"}),
                 lambda: store.max_marginal_relevance_search_by_vector(store.embedding.embed_query("x"), 3, filter={"tenant": "a"})):
        with pytest.raises(RarcUnsupported, match="similarity"):
            call()
    f8 = HipFlatVectorStore(HashEmbeddings(64), metric="cosine", storage="f8")
    f8.add_texts(["a", "b", "c"], [{"tenant": "a"}] * 3)
    for call in (lambda: f8.similarity_search("a", 2, filter={"tenant": "a"}), lambda: f8.row_filter({"tenant": "a"}),
                 lambda: f8.batch_similarity_search(["a"], 2, filter={"tenant": "a"})):
        with pytest.raises(RarcUnsupported, match="'f16' or 'f32'"):
            call()
    assert len(f8.similarity_search("a", 2)) == 2
    sharded = HipShardedFlatVectorStore(HashEmbeddings(64), metric="cosine")       # (refused before anything is looked at)
    for call in (lambda: sharded.similarity_search("a", 2, filter={"tenant": "a"}),
                 lambda: sharded.similarity_search_by_vector(sharded.embedding.embed_query("a"), 2, filter={"tenant": "a"}),
                 lambda: sharded.batch_similarity_search_with_score(["a"], 2, filter={"tenant": "a"}),
                 lambda: sharded.row_filter({"tenant": "a"})):
        with pytest.raises(RarcUnsupported, match="one-GPU store"):
            call()
