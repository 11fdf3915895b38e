"""HipGraphRetriever on the GPU: the chunks EntityGraph.retrieve_chunks ranks, as Documents that carry their score; the batch
entry point against invoke; the registered config against the retriever built from arrays; and the graph as an arm of
MultiPathRetriever beside a dense one, fused by RRF."""
import json

import numpy as np
import pytest

from tests import passage_ref as P
from tests import ppr_ref as R
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu

N_ENT, N_CHUNKS, DIM = 40, 30, 64
ENTITIES = [f"entity {i}" for i in range(N_ENT)]
CHUNKS = [f"chunk {i} of the corpus" for i in range(N_CHUNKS)]
IDS = [f"c{i}" for i in range(N_CHUNKS)]
QUERIES = ["entity 3", "entity 17", "who founded entity 5", "entity 39", "an unrelated question"]
EDGES, EDGE_W = R.random_graph(N_ENT, 90, seed=21, max_weight=4)
MENTIONS, MENTION_W = P.random_mentions(N_ENT, N_CHUNKS, seed=22, max_degree=4, max_weight=9)


@pytest.fixture(scope="module")
def world():
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    emb = HashEmbeddings(DIM)
    x = np.asarray(emb.embed_documents(ENTITIES), np.float32)
    retriever = HipGraphRetriever.from_arrays(emb, x, EDGES, MENTIONS, CHUNKS, pair_weights=EDGE_W, mention_weights=MENTION_W, ids=IDS, k=5)
    return emb, x, retriever


def test_invoke_returns_the_chunks_retrieve_chunks_ranks_with_their_scores(world):
    emb, x, r = world
    q = np.asarray([emb.embed_query(t) for t in QUERIES], np.float32)
    ids, sc, cnt = r.graph.retrieve_chunks(r.index, q, r.mentions, seeds_per_query=5, top_k=7)
    D, I = r.index.search(q, 5)
    for i, text in enumerate(QUERIES):
        docs = r.invoke(text, k=7)
        assert [d.id for d in docs] == [IDS[c] for c in ids[i, :cnt[i]]] and [d.score for d in docs] == sc[i, :cnt[i]].tolist()
        assert [d.content for d in docs] == [CHUNKS[c] for c in ids[i, :cnt[i]]]
        w = R.quantise_weights(np.clip(D[i].astype(np.float64), 0.0, None))                   # and those are the reference's
        p, _ = R.ppr_one(N_ENT, EDGES, I[i].tolist(), w, weights=EDGE_W)
        wi, wsc, wc = P.topk(P.chunk_state(p, N_CHUNKS, MENTIONS, MENTION_W), 7)
        assert [d.id for d in docs] == [IDS[c] for c in wi[:wc]] and [d.score for d in docs] == wsc[:wc]
    assert I[0, 0] == 3 and len(r.invoke(QUERIES[0])) == 5          # the entity's own text leads its seeds; k defaults to the retriever's
    assert not hasattr(r.docs[0], "score")                          # the stored chunks are not touched


def test_batch_invoke_equals_invoke(world):
    _, _, r = world
    batch = r.batch_invoke(QUERIES, k=6)
    for text, docs in zip(QUERIES, batch):
        one = r.invoke(text, k=6)
        assert [(d.id, d.content, d.score) for d in docs] == [(d.id, d.content, d.score) for d in one] and len(one) > 0
    assert r.batch_invoke([]) == []


def test_k_beyond_the_scored_chunks_returns_the_count_not_padding(world):
    _, _, r = world
    scored = int((r.graph.retrieve_chunks(r.index, np.asarray([r.embedding.embed_query(QUERIES[1])], np.float32), r.mentions,
                                          top_k=N_CHUNKS)[2])[0])
    empty = N_CHUNKS - len({c for c, _ in MENTIONS})
    assert empty > 0 and 0 < scored <= N_CHUNKS - empty
    for k in (N_CHUNKS, N_CHUNKS + 20, 10_000):
        docs = r.invoke(QUERIES[1], k=k)
        assert len(docs) == scored and all(d.score > 0 for d in docs)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must be > 0"):
            r.invoke(QUERIES[1], k=bad)


def _write_world(tmp_path, emb, x):
    np.savez(tmp_path / "graph.npz", pairs=np.asarray(EDGES, np.int64), pair_weights=np.asarray(EDGE_W, np.int64),
             mentions=np.asarray(MENTIONS, np.int64), mention_weights=np.asarray(MENTION_W, np.int64), entity_embeddings=x,
             texts=np.array(CHUNKS), ids=np.array(IDS))
    np.savez(tmp_path / "emb.npz", texts=np.array(QUERIES + CHUNKS), vectors=np.asarray(emb.embed_documents(QUERIES + CHUNKS), np.float32))
    return {"type": "hip_graph_retriever", "graph_path": str(tmp_path / "graph.npz"), "k": 5,
            "embedding": {"type": "table_embeddings", "path": str(tmp_path / "emb.npz")}}


def test_the_registered_config_answers_as_the_retriever_built_from_arrays(world, tmp_path):
    from rag_arc_amd.config.app_registration import register_graph_retriever, registrator

    emb, x, r = world
    (tmp_path / "graph.json").write_text(json.dumps(_write_world(tmp_path, emb, x)))
    register_graph_retriever(str(tmp_path / "graph.json"), "t_graph_retriever")
    app = registrator.get_object("t_graph_retriever")
    for text in QUERIES:
        got, want = app.invoke(text, k=8), r.invoke(text, k=8)
        assert [(d.id, d.content, d.score) for d in got] == [(d.id, d.content, d.score) for d in want] and got
    assert [[d.id for d in docs] for docs in app.batch_invoke(QUERIES)] == [[d.id for d in r.invoke(t)] for t in QUERIES]


def test_the_graph_as_an_arm_of_multipath_beside_a_dense_one(world, tmp_path):
    from rag_arc_amd.config.app_registration import register_multipath_retriever, registrator
    from rag_arc_amd.core.utils.fusion import RetrievalResult, RRFusion

    emb, x, _ = world
    graph_cfg = _write_world(tmp_path, emb, x)
    np.savez(tmp_path / "corpus.npz", texts=np.array(CHUNKS), ids=np.array(IDS))
    dense_cfg = {"type": "vectorstore_retriever",
                 "vectorstore": {"type": "hip_flat_vectorstore", "metric": "cosine", "corpus_path": str(tmp_path / "corpus.npz"),
                                 "embedding": {"type": "table_embeddings", "path": str(tmp_path / "emb.npz")}}}
    cfg = {"type": "multipath_retriever", "top_k_per_retriever": 12, "fusion": {"type": "rrf", "k": 60.0},
           "retrievers": [dense_cfg, graph_cfg]}
    (tmp_path / "hybrid.json").write_text(json.dumps(cfg))
    register_multipath_retriever(str(tmp_path / "hybrid.json"), "t_hybrid_graph")
    app = registrator.get_object("t_hybrid_graph")
    dense, graph = app.retrievers
    assert type(graph).__name__ == "HipGraphRetriever"
    for text in QUERIES:
        arms = [[RetrievalResult(document=d, score=getattr(d, "score", 1.0), rank=i + 1) for i, d in enumerate(arm.invoke(text, k=12))]
                for arm in (dense, graph)]
        assert len(arms[0]) == 12 and 0 < len(arms[1]) <= 12
        want = [r.document for r in RRFusion(k=60.0).fuse(arms, 10)]
        got = app.invoke(text, top_k=10)
        assert [(d.id, d.content) for d in got] == [(d.id, d.content) for d in want] and len(got) == 10
    assert [[d.id for d in docs] for docs in app.batch_invoke(QUERIES, top_k=10)] == [[d.id for d in app.invoke(t, top_k=10)] for t in QUERIES]
