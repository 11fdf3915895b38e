"""Batched MMR and batched relevance scores without a GPU: the C-ABI argument checks of rarc_mmr_select_rows (nothing is
launched on a refused call, so a CPU box can ask), and the store's / retriever's batch entry points on an OracleIndex store (no
native library: the MMR batch answers query by query through the single call; the relevance batch is host code anyway)."""
import ctypes
import warnings

import numpy as np
import pytest

from tests.helpers import HashEmbeddings, OracleIndex
from rag_arc_amd.core.retrieval.dense import VectorStoreRetriever
from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
from rag_arc_amd.hip import binding as B

P = ctypes.c_void_p(4096)        # a non-null, 16-byte aligned address nobody dereferences: every call below is refused


def _call(lib, rows=P, fmt=0, scales=None, n_rows=100, d_pad=128, d=64, queries=P, ldq=64, nq=4, ids=P, n=20, id_base=0,
          normalize=1, k=5, lam=0.5, out=P, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.rarc_mmr_rows_workspace_bytes(nq, n, d)
    return lib.rarc_mmr_select_rows(rows, fmt, scales, n_rows, d_pad, d, queries, ldq, nq, ids, n, id_base, normalize, k, lam, out,
                                    ws, ws_bytes, None)


def test_mmr_select_rows_validates_its_arguments_without_a_gpu():
    lib = B.load_library()
    for name in ("rows", "queries", "ids", "out", "ws"):
        assert _call(lib, **{name: None}) == -1 and b"null pointer" in lib.rarc_last_error(), name
    for bad in (dict(n=0), dict(d=0), dict(d=129), dict(d_pad=120, d=64), dict(ldq=63), dict(k=0), dict(nq=-1), dict(n_rows=-1)):
        assert _call(lib, ws_bytes=1 << 30, **bad) == -1 and b"bad sizes" in lib.rarc_last_error(), bad
    assert _call(lib, n=1025, ws_bytes=1 << 40) == -4 and b"1024" in lib.rarc_last_error()          # MMR_MAX_N
    assert _call(lib, fmt=3) == -1 and b"row format" in lib.rarc_last_error()
    assert _call(lib, fmt=-1) == -1 and b"row format" in lib.rarc_last_error()
    assert _call(lib, fmt=1, d_pad=256) == -1 and b"row scales" in lib.rarc_last_error()
    assert _call(lib, rows=ctypes.c_void_p(4104)) == -1 and b"aligned" in lib.rarc_last_error()
    need = lib.rarc_mmr_rows_workspace_bytes(4, 20, 64)
    assert _call(lib, ws_bytes=need - 1) == -3 and b"workspace" in lib.rarc_last_error()
    assert _call(lib, ws=ctypes.c_void_p(4100)) == -3
    with pytest.raises(B.RarcError, match="rarc_mmr_select_rows"):
        B.check(_call(lib, ws_bytes=0), "rarc_mmr_select_rows")


def test_mmr_rows_workspace_bytes():
    lib = B.load_library()
    assert lib.rarc_mmr_rows_workspace_bytes(1, 20, 768) == (20 * 768 + 768) * 8
    assert lib.rarc_mmr_rows_workspace_bytes(256, 20, 768) == 256 * (20 * 768 + 768) * 8
    assert lib.rarc_mmr_rows_workspace_bytes(7, 1024, 4096) == 7 * (1024 * 4096 + 4096) * 8       # (size_t arithmetic: 235 MB)
    for nq, n, d in ((0, 20, 64), (-1, 20, 64), (4, 0, 64), (4, 1025, 64), (4, 20, 0), (4, 20, -3)):
        assert lib.rarc_mmr_rows_workspace_bytes(nq, n, d) == 0, (nq, n, d)


def _store(n=300, dim=32, metric="cosine"):
    store = HipFlatVectorStore(HashEmbeddings(dim), metric=metric, engine_factory=lambda d, m, dev: OracleIndex(d, m, dev))
    store.add_texts([f"text number {i}" for i in range(n)], ids=[str(i) for i in range(n)])
    return store


QUERIES = [f"topic {i}" for i in range(7)]


def _cutting_threshold(store, k=6):
    """A relevance threshold that some of the batch's answers pass and some do not: the median relevance score, clamped to the
    [0, 1] the retriever accepts."""
    scores = sorted(s for q in QUERIES for _, s in store.similarity_search_with_relevance_scores(q, k=k))
    return min(1.0, max(0.0, float(scores[len(scores) // 2])))


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_batch_relevance_scores_equal_the_single_calls_warnings_included(metric):
    store = _store(metric=metric)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mid = _cutting_threshold(store)
    warned = 0
    for kw in ({}, {"score_threshold": 0.0}, {"score_threshold": mid}, {"score_threshold": 1.0}):
        with warnings.catch_warnings(record=True) as w_one:
            warnings.simplefilter("always")
            want = [store.similarity_search_with_relevance_scores(q, k=6, **kw) for q in QUERIES]
        with warnings.catch_warnings(record=True) as w_batch:
            warnings.simplefilter("always")
            got = store.batch_similarity_search_with_relevance_scores(QUERIES, k=6, **kw)
        assert [[(d.id, s) for d, s in a] for a in got] == [[(d.id, s) for d, s in a] for a in want], (metric, kw)
        assert len(w_batch) == len(w_one), (metric, kw)
        warned += len(w_batch)
    assert store.batch_similarity_search_with_relevance_scores([], k=3) == []
    if metric == "cosine":
        cut = sum(len(a) for a in store.batch_similarity_search_with_relevance_scores(QUERIES, k=6, score_threshold=mid))
        assert 0 < cut < 6 * len(QUERIES), cut
    else:                       # (raw inner products of unnormalised vectors: relevance outside [0, 1], one warning per query)
        assert warned


def test_batch_mmr_on_an_engine_without_the_library_equals_the_single_calls():
    store = _store()
    for kw in ({}, {"reembed": False}, {"reembed": False, "fetch_k": 400}, {"k": 20, "fetch_k": 20}, {"lambda_mult": 0.0}):
        want = [[d.id for d in store.max_marginal_relevance_search(q, **kw)] for q in QUERIES]
        assert [[d.id for d in a] for a in store.batch_max_marginal_relevance_search(QUERIES, **kw)] == want, kw
        vecs = [store.embedding.embed_query(q) for q in QUERIES]
        assert [[d.id for d in a] for a in store.batch_max_marginal_relevance_search_by_vector(vecs, **kw)] == want, kw
    assert store.mmr_stats == {"batched_calls": 0, "batched_queries": 0, "fallback_queries": 10 * len(QUERIES)}
    assert store.batch_max_marginal_relevance_search([], k=3) == []
    empty = HipFlatVectorStore(HashEmbeddings(32), engine_factory=lambda d, m, dev: OracleIndex(d, m, dev))
    assert empty.batch_max_marginal_relevance_search(QUERIES, reembed=False) == [[] for _ in QUERIES]
    assert empty.batch_similarity_search_with_relevance_scores(QUERIES) == [[] for _ in QUERIES]


def test_batch_mmr_refuses_filters():
    store = _store()
    searches = []

    def search(*a, **kw):
        searches.append(a)
        raise AssertionError("a refused call reached the index")

    store.index.search = search
    for kw in ({"filter": {"a": 1}}, {"filters": [None] * 6 + [{"a": 1}]}, {"filters": [lambda md: True] * 7}):
        with pytest.raises(B.RarcUnsupported, match="max_marginal_relevance_search"):
            store.batch_max_marginal_relevance_search(QUERIES, **kw)
        with pytest.raises(B.RarcUnsupported, match="max_marginal_relevance_search"):
            store.batch_max_marginal_relevance_search_by_vector([[0.0] * 32] * 7, **kw)
    assert not searches
    r = VectorStoreRetriever(store, search_type="mmr")
    with pytest.raises(B.RarcUnsupported):
        r.batch_invoke(QUERIES, filters=[{"a": 1}] * 7)
    with pytest.raises(B.RarcUnsupported):
        r.invoke(QUERIES[0], filter={"a": 1})


def test_batch_invoke_goes_through_the_batch_entry_points():
    store = _store()
    seen = []
    for name in ("batch_max_marginal_relevance_search", "batch_similarity_search_with_relevance_scores"):
        inner = getattr(store, name)
        setattr(store, name, lambda *a, _inner=inner, _name=name, **kw: seen.append(_name) or _inner(*a, **kw))
    r = VectorStoreRetriever(store, search_type="mmr", search_kwargs={"fetch_k": 30, "reembed": False})
    assert [[d.id for d in a] for a in r.batch_invoke(QUERIES, k=6)] == [[d.id for d in r.invoke(q, k=6)] for q in QUERIES]
    for thr in (0.0, _cutting_threshold(store)):
        r = VectorStoreRetriever(store, search_type="similarity_score_threshold", search_kwargs={"score_threshold": thr})
        got = [[d.id for d in a] for a in r.batch_invoke(QUERIES, k=6)]
        assert got == [[d.id for d in r.invoke(q, k=6)] for q in QUERIES]
    assert any(len(a) < 6 for a in got) and any(a for a in got)          # (the second threshold cuts some answers, not all)
    assert seen == ["batch_max_marginal_relevance_search"] + ["batch_similarity_search_with_relevance_scores"] * 2


def test_the_sharded_store_has_no_batched_mmr():
    from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import HipShardedFlatVectorStore as S

    for name in ("batch_max_marginal_relevance_search", "batch_max_marginal_relevance_search_by_vector",
                 "batch_similarity_search_with_relevance_scores"):
        assert getattr(S, name, None) is None, name
    assert getattr(S, "batch_similarity_search", None) is not None


class _NativeLikeIndex(OracleIndex):
    """An OracleIndex with the surface the batched MMR path asks of the default engine (`lib`, search_device,
    mmr_select_device), computed on the host: what the store does AROUND the two launches can then be checked without a GPU."""
    lib = object()

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def search_device(self, q, k):
        import torch

        self.calls.append(("search_device", len(q), k))
        scores, ids = self.search(np.asarray(q, np.float32), k)
        return torch.from_numpy(np.asarray(ids, np.int64)), torch.from_numpy(np.asarray(scores, np.float32))

    def mmr_select_device(self, q64, cand_ids, k, lambda_mult=0.5, normalize=None):
        import torch

        from rag_arc_amd.encapsulation.database.vector_db.hip_flat import _mmr_select

        self.calls.append(("mmr_select_device", len(q64), k))
        out = np.full((len(q64), k), -1, np.int64)
        for i, (q, ids) in enumerate(zip(np.asarray(q64, np.float64), cand_ids.numpy())):
            ids = ids[ids >= 0]
            cand = self._rows[ids].view(np.float16).astype(np.float32)[:, : self.dim].astype(np.float64)
            if normalize:
                q, cand = q / np.linalg.norm(q), cand / np.linalg.norm(cand, axis=1, keepdims=True)
            picks = _mmr_select([(int(r), 0.0) for r in ids], cand.tolist(), q.tolist(), k, lambda_mult)
            out[i, : len(picks)] = picks
        return torch.from_numpy(out)


def test_the_batched_path_around_its_two_launches():
    """300 queries: two passes, each one search_device for min(fetch_k, ntotal) candidates and one mmr_select_device; the
    selected rows map to the documents the single call (host selection over the same stored rows) returns."""
    plain = _store(n=90)
    fast = HipFlatVectorStore(HashEmbeddings(32), engine_factory=lambda d, m, dev: _NativeLikeIndex(d, m, dev))
    fast.add_texts([f"text number {i}" for i in range(90)], ids=[str(i) for i in range(90)])
    queries = [f"topic {i}" for i in range(300)]
    for k, fetch_k in ((5, 20), (20, 20), (4, 700)):
        want = [[d.id for d in plain.max_marginal_relevance_search(q, k=k, fetch_k=fetch_k, reembed=False)] for q in queries]
        del fast.index.calls[:]
        got = fast.batch_max_marginal_relevance_search(queries, k=k, fetch_k=fetch_k, reembed=False)
        assert [[d.id for d in a] for a in got] == want, (k, fetch_k)
        n = min(fetch_k, 90)
        assert fast.index.calls == [("search_device", 256, n), ("mmr_select_device", 256, min(k, n)),
                                    ("search_device", 44, n), ("mmr_select_device", 44, min(k, n))]
    assert fast.mmr_stats == {"batched_calls": 3, "batched_queries": 900, "fallback_queries": 0}
