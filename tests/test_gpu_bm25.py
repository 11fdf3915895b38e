"""BM25 on the MI355X: rarc_bm25_scores / rarc_bm25_topk against the restatement of rank_bm25's BM25Okapi (fp64 bits),
the retriever's surface, and the hybrid (dense + BM25 + RRF) retriever built from JSON."""
import asyncio
import json

import numpy as np
import pytest

from rag_arc_amd.core.retrieval.base import BaseRetriever
from rag_arc_amd.core.retrieval.bm25 import HipBM25Retriever
from rag_arc_amd.hip.bm25 import (Bm25Device, Bm25Index, OkapiRestatement, synthetic_zipf, topk_order, zipf_terms)
from tests.helpers import HashEmbeddings, OracleFusion, OracleIndex

pytestmark = pytest.mark.gpu


def hexes(a):
    return [float(x).hex() for x in np.asarray(a, dtype=np.float64).ravel()]


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def corpus_lists(off, ids):
    return [ids[off[d]:off[d + 1]].tolist() for d in range(off.size - 1)]


def check_topk(dev, idx, queries, k):
    got_i, got_s = dev.topk(queries, k)
    for q, terms in enumerate(queries):
        sc = idx.host_scores(terms)
        want = topk_order(sc, k)
        assert np.array_equal(got_i[q], want), (q, k, got_i[q][:10], want[:10])
        assert same_bits(got_s[q], sc[want]), (q, k)


HAND = [("a b", "a c", "a b d"), ("x y y", "y z", "w", "x x x z"), ("café 東京 東京", "naïve café", "東京")]


@pytest.mark.parametrize("texts", HAND)
def test_hand_cases_scores_bit_identical(texts):
    r = HipBM25Retriever.from_texts(list(texts), warn_default_preprocess=False)
    ref = OkapiRestatement([t.split() for t in texts])
    words = sorted(ref.idf) + ["unknown"]
    for q in [[w] for w in words] + [words, words[:2] * 3, ["unknown"]]:
        assert hexes(r.get_scores(" ".join(q))) == hexes(ref.get_scores(q)), q
        pairs = r.get_top_k_with_scores(" ".join(q), k=10)
        want = topk_order(ref.get_scores(q), 10)
        assert [d.content for d, _ in pairs] == [texts[i] for i in want]
        assert all(type(s) is float for _, s in pairs)
        assert hexes([s for _, s in pairs]) == hexes(ref.get_scores(q)[want])


def test_negative_epsilon_ranks_untouched_documents_first():
    r = HipBM25Retriever.from_texts(["a b", "a c", "a b d"], warn_default_preprocess=False)
    sc = r.get_scores("b")
    assert sc[1] == 0.0 and sc[0] < 0 and sc[2] < 0
    assert [d.content for d in r.invoke("b", k=3)] == ["a c", "a b d", "a b"]


def test_zipf_20k_scores_bit_identical():
    off, ids = synthetic_zipf(20_000, 30, 50_000, seed=7)
    idx = Bm25Index.from_token_ids(off, ids, n_terms=50_000)
    ref = OkapiRestatement(corpus_lists(off, ids))
    dev = Bm25Device(idx)
    rng = np.random.default_rng(1)
    queries = [idx.known_ids(zipf_terms(rng, int(rng.integers(1, 12)), 50_000)) for _ in range(12)]
    queries += [[0, 0, 0], [int(np.argmax(idx.post_off[1:] - idx.post_off[:-1]))], []]
    got = dev.scores(queries)
    for q, terms in enumerate(queries):
        assert same_bits(got[q], ref.get_scores(terms)), q
        assert same_bits(got[q], idx.host_scores(terms)), q


def _mixed_corpus():
    """20k documents over three 8192-document tiles: term 0 in every document, term 1 only in the four documents on the
    two sides of the tile boundaries, terms >= 2 from a Zipf body."""
    rng = np.random.default_rng(11)
    off, ids = synthetic_zipf(20_000, 20, 5_000, seed=3)
    docs = corpus_lists(off, ids + 2)
    for d in range(len(docs)):
        docs[d] = [0] + docs[d]
    for d in (8191, 8192, 16383, 16384):             # both sides of the tile boundaries share a rare term
        docs[d] = docs[d] + [1, 1]
    lens = [len(x) for x in docs]
    return np.cumsum([0] + lens), np.array([t for x in docs for t in x]), rng


@pytest.mark.parametrize("nq", [1, 7, 256, 300])
def test_topk_against_the_restatement(nq):
    off, ids, rng = _mixed_corpus()
    idx = Bm25Index.from_token_ids(off, ids)
    dev = Bm25Device(idx)
    queries = [idx.known_ids(zipf_terms(rng, int(rng.integers(1, 9)), 5_000) + 2) for _ in range(nq)]
    queries[0] = [1]                                  # the rare term at the tile boundaries
    if nq > 1:
        queries[1] = []                               # no known token: the first k documents, score 0
    if nq > 2:
        queries[2] = [0, 1, 0]                        # the term every document has, repeated
    for k in (1, 5, 50, 100, 1000):
        check_topk(dev, idx, queries, k)
    got_i, got_s = dev.topk(queries[:2], 5)
    assert sorted(got_i[0].tolist()[:4]) == [8191, 8192, 16383, 16384] and got_s[0][3] > got_s[0][4]


def test_topk_small_corpus_k_beyond_n_and_empty_documents():
    rng = np.random.default_rng(4)
    docs = [[] if d % 7 == 0 else rng.integers(0, 40, size=int(rng.integers(1, 9))).tolist() for d in range(700)]
    off = np.cumsum([0] + [len(x) for x in docs])
    idx = Bm25Index.from_token_ids(off, [t for x in docs for t in x])
    dev = Bm25Device(idx)
    queries = [idx.known_ids(rng.integers(0, 40, size=3)) for _ in range(9)] + [[]]
    check_topk(dev, idx, queries, 5000)               # effective k = 700: every document, empty ones included
    check_topk(dev, idx, queries, 1)


def test_negative_epsilon_corpus_across_tiles():
    """Four common words (every idf negative, so eps < 0): documents with none of them (0.0) outrank all others."""
    rng = np.random.default_rng(8)
    docs = [[w for w in range(4) if rng.random() < 0.7] for _ in range(9000)]
    off = np.cumsum([0] + [len(x) for x in docs])
    idx = Bm25Index.from_token_ids(off, [t for x in docs for t in x])
    assert idx.average_idf < 0
    dev = Bm25Device(idx)
    queries = [[0], [1, 2], [3, 3, 0], [0, 1, 2, 3]]
    check_topk(dev, idx, queries, 100)
    untouched = [d for d in range(9000) if 0 not in docs[d]]
    ids, sc = dev.topk([[0]], 100)
    assert ids[0].tolist() == untouched[:100] and not sc[0].any()
    ref = OkapiRestatement(docs)
    assert same_bits(dev.scores(queries), np.stack([ref.get_scores(q) for q in queries]))


TEXTS = [f"doc {i} " + " ".join(f"w{(i * j) % 97}" for j in range(1, 2 + i % 9)) for i in range(3000)]
QUERIES = ["w3 w5", "doc w17 w17", "nothing here", "w0", "w96 w95 w1 doc"]


def _retriever(texts=TEXTS, **kw):
    return HipBM25Retriever.from_texts(texts, ids=[f"id{i}" for i in range(len(texts))], warn_default_preprocess=False,
                                       **kw)


def test_invoke_batch_invoke_ainvoke_agree_and_runs_repeat():
    r = _retriever(k=7)
    one = [[d.id for d in r.invoke(q)] for q in QUERIES]
    batch = [[d.id for d in docs] for docs in r.batch_invoke(QUERIES)]

    async def run():
        return [[d.id for d in await r.ainvoke(q)] for q in QUERIES]

    assert one == batch == asyncio.run(run())
    ref = OkapiRestatement([t.split() for t in TEXTS])
    assert one == [[f"id{i}" for i in topk_order(ref.get_scores(q.split()), 7)] for q in QUERIES]
    assert [len(d) for d in r.batch_invoke(QUERIES, k=20)] == [20] * len(QUERIES)
    a = [r.get_top_k_with_scores(q, k=50) for q in QUERIES]
    b = [r.get_top_k_with_scores(q, k=50) for q in QUERIES]
    assert [[(d.id, s.hex()) for d, s in x] for x in a] == [[(d.id, s.hex()) for d, s in x] for x in b]
    assert r.get_name() == "BM25Retriever"
    info = r.get_bm25_info()
    assert info["document_count"] == 3000 and info["vocab_size"] == len(ref.idf) and info["average_doc_length"] == ref.avgdl


def test_add_and_delete_equal_a_fresh_build():
    from rag_arc_amd.core.utils.data_model import Document

    r = _retriever(TEXTS[:2000])
    added = r.add_documents([Document(content=t, metadata={}, id=f"id{i}") for i, t in enumerate(TEXTS[2000:], 2000)],
                            rebuild_threshold=10 ** 6)
    assert len(added) == 1000
    fresh = _retriever()
    for q in QUERIES:
        assert [d.id for d in r.invoke(q, k=30)] == [d.id for d in fresh.invoke(q, k=30)]
        assert hexes(r.get_scores(q)) == hexes(fresh.get_scores(q))
    gone = [f"id{i}" for i in range(0, 3000, 3)]
    assert r.delete_documents(gone, rebuild_threshold=10 ** 6)
    kept = [i for i in range(3000) if i % 3]
    fresh2 = HipBM25Retriever.from_texts([TEXTS[i] for i in kept], ids=[f"id{i}" for i in kept],
                                         warn_default_preprocess=False)
    for q in QUERIES:
        assert [d.id for d in r.invoke(q, k=30)] == [d.id for d in fresh2.invoke(q, k=30)]
    assert asyncio.run(r.adelete_documents(None)) and r.get_document_count() == 0


def test_save_load_round_trip(tmp_path):
    r = _retriever(k=9, bm25_params={"k1": 1.2, "b": 0.6})
    r.save_to_disk(str(tmp_path))
    again = HipBM25Retriever.load_from_disk(str(tmp_path / "bm25.pkl"))
    assert again.k == 9 and again.bm25_params == {"k1": 1.2, "b": 0.6}
    for q in QUERIES:
        assert [d.id for d in again.invoke(q)] == [d.id for d in r.invoke(q)]
        assert hexes(again.get_scores(q)) == hexes(r.get_scores(q))


class _RestatedBM25(BaseRetriever):
    def __init__(self, texts, ids):
        super().__init__()
        from rag_arc_amd.core.utils.data_model import Document

        self.ref = OkapiRestatement([t.split() for t in texts])
        self.docs = [Document(content=t, metadata={}, id=i) for t, i in zip(texts, ids)]

    def _get_relevant_documents(self, query, **kwargs):
        k = min(kwargs.get("k", 5), len(self.docs))
        return [self.docs[i] for i in topk_order(self.ref.get_scores(query.split()), k)]


def test_hybrid_dense_bm25_rrf_from_json(tmp_path):
    from rag_arc_amd.config.app_registration import register_multipath_retriever, registrator
    from rag_arc_amd.core.retrieval import MultiPathRetriever, VectorStoreRetriever
    from rag_arc_amd.encapsulation.database.vector_db import HipFlatVectorStore
    from rag_arc_amd.encapsulation.embeddings.table import TableEmbeddings

    texts, ids = TEXTS[:2000], [str(i) for i in range(2000)]
    queries = QUERIES + ["doc 77 w3"]
    emb = HashEmbeddings(384)
    np.savez(tmp_path / "emb.npz", texts=np.array(texts + queries),
             vectors=np.array(emb.embed_documents(texts + queries), np.float32))
    np.savez(tmp_path / "corpus.npz", texts=np.array(texts), ids=np.array(ids))
    vs = {"type": "hip_flat_vectorstore", "metric": "cosine",
          "embedding": {"type": "table_embeddings", "path": str(tmp_path / "emb.npz")},
          "corpus_path": str(tmp_path / "corpus.npz")}
    cfg = {"type": "multipath_retriever", "top_k_per_retriever": 20, "fusion": {"type": "rrf", "k": 60.0},
           "retrievers": [{"type": "vectorstore_retriever", "vectorstore": vs},
                          {"type": "hip_bm25_retriever", "corpus_path": str(tmp_path / "corpus.npz")}]}
    (tmp_path / "hybrid.json").write_text(json.dumps(cfg))
    register_multipath_retriever(str(tmp_path / "hybrid.json"), "t_hybrid_bm25")
    app = registrator.get_object("t_hybrid_bm25")
    table = TableEmbeddings.from_npz(str(tmp_path / "emb.npz"))
    dense_ref = HipFlatVectorStore.from_texts(texts, table, ids=ids, engine_factory=lambda d, m, dev: OracleIndex(d, m))
    want_app = MultiPathRetriever([VectorStoreRetriever(dense_ref), _RestatedBM25(texts, ids)],
                                  fusion_method=OracleFusion(60.0), top_k_per_retriever=20)
    for q in queries:
        got = app.invoke(q, top_k=10)
        want = want_app.invoke(q, top_k=10)
        assert [(d.content, d.id) for d in got] == [(d.content, d.id) for d in want], q
    assert [[d.id for d in x] for x in app.batch_invoke(queries, top_k=10)] == \
           [[d.id for d in app.invoke(q, top_k=10)] for q in queries]


def test_one_million_documents():
    off, ids = synthetic_zipf(1_000_000, 32, 1 << 16, seed=21)
    idx = Bm25Index.from_token_ids(off, ids, n_terms=1 << 16)
    dev = Bm25Device(idx)
    rng = np.random.default_rng(22)
    queries = [idx.known_ids(zipf_terms(rng, 8, 1 << 16)) for _ in range(256)]
    check_topk(dev, idx, queries, 100)
