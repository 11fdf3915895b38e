"""Batched MMR through the store and the retriever: batch_max_marginal_relevance_search(queries, reembed=False) answers every
256 queries with one encoder call, one search for the candidates, one rarc_mmr_select_rows launch and one host mapping — and
element i is, document for document, what max_marginal_relevance_search(queries[i], ...) returns (the single call: one search,
a gather, rarc_mmr_select and a read-back per query).  The relevance-score batch and the retriever's batch_invoke likewise."""
import numpy as np
import pytest

from tests.helpers import HashEmbeddings
from rag_arc_amd.core.retrieval.dense import VectorStoreRetriever
from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
from rag_arc_amd.hip import binding as B

pytestmark = pytest.mark.gpu

N_DOCS, DIM = 600, 64
PAIRS = [(s, m) for s in ("f16", "f8", "f32") for m in ("cosine", "ip", "l2") if not (s == "f8" and m == "l2")]
QUERIES = [f"what is known about subject {i}?" for i in range(300)]          # 300: two passes of the batched path


class _CountingEmbeddings(HashEmbeddings):
    """embed_query is embed_documents([text])[0]; the batch form says so and counts its calls."""

    def __init__(self, dim):
        super().__init__(dim)
        self.batch_calls = []

    def embed_queries(self, texts):
        self.batch_calls.append(len(texts))
        return self.embed_documents(list(texts))


def _store(storage="f16", metric="cosine", n=N_DOCS):
    store = HipFlatVectorStore(_CountingEmbeddings(DIM), metric=metric, storage=storage)
    if n:
        store.add_texts([f"document number {i} about subject {i % 37}" for i in range(n)], ids=[str(i) for i in range(n)])
    return store


def _count_launches(store):
    """Counters of the engine's two entry points the batched path goes through (the engine keeps no launch counter of its own;
    a search_device call of at most 256 queries is one scan).  Counting again starts from zero and does not wrap the wrappers."""
    calls = {"search_device": 0, "mmr_select_device": 0}
    for name in calls:
        inner = getattr(store.index, name)
        inner = getattr(inner, "_counted_inner", inner)

        def counted(*a, _inner=inner, _name=name, **kw):
            calls[_name] += 1
            return _inner(*a, **kw)

        counted._counted_inner = inner
        setattr(store.index, name, counted)
    return calls


def _ids(answers):
    return [[d.id for d in docs] for docs in answers]


@pytest.mark.parametrize("storage,metric", PAIRS)
def test_batch_equals_the_single_calls_document_for_document(storage, metric):
    store = _store(storage, metric)
    for k, fetch_k in ((5, 20), (20, 20), (4, 700)):                 # (20, 20): everything is selected; 700 > ntotal
        want = _ids([store.max_marginal_relevance_search(q, k=k, fetch_k=fetch_k, reembed=False) for q in QUERIES])
        assert all(len(w) == k for w in want)
        if k < fetch_k:
            scored = _ids(store.batch_similarity_search(QUERIES, k=k))
            assert any(w != s for w, s in zip(want, scored)), "MMR never left the similarity order: the test shows nothing"
        for nq in (1, 7, 300):
            calls = _count_launches(store)
            before, embeds = dict(store.mmr_stats), len(store.embedding.batch_calls)
            got = store.batch_max_marginal_relevance_search(QUERIES[:nq], k=k, fetch_k=fetch_k, reembed=False)
            assert _ids(got) == want[:nq], (storage, metric, k, fetch_k, nq)
            passes = -(-nq // 256)
            assert calls == {"search_device": passes, "mmr_select_device": passes}
            assert store.embedding.batch_calls[embeds:] == ([256, nq - 256] if nq > 256 else [nq])
            after = store.mmr_stats
            assert after["batched_calls"] == before["batched_calls"] + 1 and after["batched_queries"] == before["batched_queries"] + nq
            assert after["fallback_queries"] == before["fallback_queries"]
        vecs = [store.embedding.embed_query(q) for q in QUERIES[:7]]
        by_vec = store.batch_max_marginal_relevance_search_by_vector(vecs, k=k, fetch_k=fetch_k, reembed=False)
        assert _ids(by_vec) == want[:7]
        assert _ids(store.batch_max_marginal_relevance_search_by_vector(np.asarray(vecs), k=k, fetch_k=fetch_k, reembed=False,
                                                                        lambda_mult=0.5)) == want[:7]
    for lam in (0.0, 1.0):
        want = _ids([store.max_marginal_relevance_search(q, k=6, fetch_k=25, lambda_mult=lam, reembed=False) for q in QUERIES[:9]])
        assert _ids(store.batch_max_marginal_relevance_search(QUERIES[:9], k=6, fetch_k=25, lambda_mult=lam, reembed=False)) == want


def test_fallbacks_and_refusals():
    store = _store()
    qs = QUERIES[:5]
    # reembed=True (the default): the reference's way, query by query
    calls = _count_launches(store)
    want = _ids([store.max_marginal_relevance_search(q, k=5, fetch_k=20) for q in qs])
    assert _ids(store.batch_max_marginal_relevance_search(qs, k=5, fetch_k=20)) == want
    assert _ids(store.batch_max_marginal_relevance_search(qs, k=5, fetch_k=20, reembed=True)) == want
    assert store.mmr_stats == {"batched_calls": 0, "batched_queries": 0, "fallback_queries": 10}
    assert calls["mmr_select_device"] == 0
    # fetch_k beyond the selection kernel's 1024 candidates: query by query as well (the single call then takes the host path
    # or refuses as it always did; a 600-row store clamps fetch_k to 600 inside the single call)
    want = _ids([store.max_marginal_relevance_search(q, k=5, fetch_k=2000, reembed=False) for q in qs])
    assert _ids(store.batch_max_marginal_relevance_search(qs, k=5, fetch_k=2000, reembed=False)) == want
    assert store.mmr_stats["fallback_queries"] == 15 and store.mmr_stats["batched_calls"] == 0
    # filter= / filters=: refused before any launch, as the single call refuses filter=
    calls = _count_launches(store)
    for kw in ({"filter": {"a": 1}}, {"filters": [{"a": 1}] * 5}, {"filters": [None, None, lambda md: True, None, None]}):
        with pytest.raises(B.RarcUnsupported, match="max_marginal_relevance_search"):
            store.batch_max_marginal_relevance_search(qs, k=5, fetch_k=20, reembed=False, **kw)
    assert calls == {"search_device": 0, "mmr_select_device": 0}
    got = store.batch_max_marginal_relevance_search(qs, k=5, fetch_k=20, reembed=False, filters=[None] * 5)     # the unfiltered batch
    assert _ids(got) == _ids([store.max_marginal_relevance_search(q, k=5, fetch_k=20, reembed=False) for q in qs])
    # an empty store
    empty = _store(n=0)
    assert empty.batch_max_marginal_relevance_search(qs, reembed=False) == [[] for _ in qs]
    assert empty.batch_max_marginal_relevance_search_by_vector([[0.0] * DIM] * 3, reembed=False) == [[], [], []]
    emptied = _store(n=50)
    emptied.delete(None)
    assert emptied.batch_max_marginal_relevance_search(qs, reembed=False) == [[] for _ in qs]
    assert store.batch_max_marginal_relevance_search([], reembed=False) == []


def test_retriever_batch_invoke_equals_invoke_one_by_one():
    store = _store()
    qs = QUERIES[:40]
    r = VectorStoreRetriever(store, search_type="mmr", search_kwargs={"fetch_k": 30, "reembed": False})
    want = _ids([r.invoke(q, k=6) for q in qs])
    before = dict(store.mmr_stats)
    assert _ids(r.batch_invoke(qs, k=6)) == want and all(len(w) == 6 for w in want)
    assert store.mmr_stats["batched_queries"] == before["batched_queries"] + 40
    with pytest.raises(B.RarcUnsupported):
        r.batch_invoke(qs, filters=[{"a": 1}] * 40)
    with pytest.raises(B.RarcUnsupported):
        r.invoke(qs[0], filter={"a": 1})
    scores = sorted(s for q in qs for _, s in store.similarity_search_with_relevance_scores(q, k=6))
    cutting = float(scores[len(scores) // 2])
    assert 0.0 < cutting < 1.0
    for thr in (0.0, cutting):
        r = VectorStoreRetriever(store, search_type="similarity_score_threshold", search_kwargs={"score_threshold": thr})
        want = _ids([r.invoke(q, k=6) for q in qs])
        assert _ids(r.batch_invoke(qs, k=6)) == want
        pairs = store.batch_similarity_search_with_relevance_scores(qs, k=6, score_threshold=thr)
        one = [store.similarity_search_with_relevance_scores(q, k=6, score_threshold=thr) for q in qs]
        assert [[(d.id, s) for d, s in a] for a in pairs] == [[(d.id, s) for d, s in a] for a in one]
    assert 0 < sum(len(w) for w in want) < 6 * len(qs)                       # (the second threshold cut some answers)
    # filter= passes through to the batched similarity search
    store2 = HipFlatVectorStore(_CountingEmbeddings(DIM))
    store2.add_texts([f"document number {i}" for i in range(90)], [{"group": i % 3} for i in range(90)], ids=[str(i) for i in range(90)])
    got = store2.batch_similarity_search_with_relevance_scores(qs[:6], k=4, filter={"group": 1})
    one = [store2.similarity_search_with_relevance_scores(q, k=4, filter={"group": 1}) for q in qs[:6]]
    assert [[(d.id, s) for d, s in a] for a in got] == [[(d.id, s) for d, s in a] for a in one]
    assert all(d.metadata["group"] == 1 for a in got for d, _ in a)
