"""Graph ingest through the public surface (graph_db/ingest.py): EntityGraph.from_rows / .extended and
MentionMap.from_rows / .extended against the host constructors on the same rows — the resident lists and the answers of the queries
built on them, element for element — RelationList.extended, both on_invalid modes, every refusal, and
HipGraphRetriever.add_documents against a retriever built from all the data at once."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: torch brings the HIP runtime both must share)

from tests import ingest_ref as R

pytestmark = pytest.mark.gpu

N = 300


def _db():
    from rag_arc_amd.encapsulation.database import graph_db

    return graph_db


def _B():
    from rag_arc_amd.hip import binding

    return binding


def _rows(seed, n=N, r=2500):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, r)
    b = (a + 1 + rng.integers(0, n - 1, r)) % n                     # any orientation, duplicates, never a == b
    return np.stack([a, b], axis=1).astype(np.int64), rng.integers(1, 30, r), rng.integers(0, 32, r)


def _host(x, unsigned=True):
    if x is None:
        return None
    x = x.cpu().numpy()
    return x.view(np.uint32) if unsigned and x.dtype == np.int32 else x


def _same_graph(a, b):
    assert (a.n, a.m) == (b.n, b.m) and a.typed == b.typed
    assert np.array_equal(_host(a._pairs), _host(b._pairs))
    for x, y in ((a._pair_weights, b._pair_weights), (a._type_masks, b._type_masks)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(_host(x), _host(y)))


def _same_map(a, b):
    assert (a.n_chunks, a.n_entities, a.nnz, a.n_split) == (b.n_chunks, b.n_entities, b.nnz, b.n_split)
    for x, y in ((a._row_ptr, b._row_ptr), (a._ent, b._ent), (a._w, b._w), (a._split, b._split)):
        assert (x is None) == (y is None) and (x is None or np.array_equal(_host(x), _host(y)))


def _same_answers(a, b, typed):
    seeds = [[0, 5], [17], [299, 3, 150], []]
    assert np.array_equal(a.personalized_pagerank(seeds), b.personalized_pagerank(seeds))
    for x, y in zip(a.personalized_pagerank(seeds, top_k=20), b.personalized_pagerank(seeds, top_k=20)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.neighbourhood(seeds, hops=2), b.neighbourhood(seeds, hops=2))
    if typed:
        filters = [[0, 1, 2], [31], list(range(16)), [7]]
        assert np.array_equal(a.neighbourhood(seeds, hops=3, relation_types=filters), b.neighbourhood(seeds, hops=3, relation_types=filters))
        assert np.array_equal(a.personalized_pagerank(seeds, relation_types=[3, 4, 5, 6]), b.personalized_pagerank(seeds, relation_types=[3, 4, 5, 6]))
    ca, cb = a.components(), b.components()
    assert np.array_equal(ca.labels, cb.labels) and ca.n_components == cb.n_components and ca.largest == cb.largest


# ---- from_rows and extended against the host constructor -------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("typed", [False, True])
def test_from_rows_equals_the_host_constructor(weighted, typed):
    rows, w, t = _rows(1)
    w, t = (w if weighted else None), (t if typed else None)
    want = _db().EntityGraph(N, rows, weights=w, types=t)
    got = _db().EntityGraph.from_rows(N, rows, weights=w, types=t)
    _same_graph(got, want)
    assert got.skipped == dict.fromkeys(R.PAIR_KINDS, 0)
    _same_answers(got, want, typed)
    # device rows, weights and types: used where they are
    dev = lambda x, dt: None if x is None else torch.from_numpy(np.asarray(x).astype(dt)).cuda()      # noqa: E731
    _same_graph(_db().EntityGraph.from_rows(N, dev(rows, np.int64), weights=dev(w, np.int32), types=dev(t, np.int32)), want)


@pytest.mark.parametrize("base_weighted, rows_weighted, typed", [(True, True, True), (False, False, False), (True, False, False), (False, True, True)])
def test_extended_equals_the_host_constructor_on_the_concatenated_rows(base_weighted, rows_weighted, typed):
    rows0, w0, t0 = _rows(2, r=1500)
    rows1, w1, t1 = _rows(3, n=N + 40, r=1200)
    one = lambda k: np.ones(k, np.int64)                                # noqa: E731  (the side without weights counts 1 a row)
    base = _db().EntityGraph(N, rows0, weights=w0 if base_weighted else None, types=t0 if typed else None)
    before = _host(base._pairs).copy()
    got = base.extended(rows1, weights=w1 if rows_weighted else None, types=t1 if typed else None, n=N + 40)
    all_w = None if not (base_weighted or rows_weighted) else np.concatenate([w0 if base_weighted else one(1500), w1 if rows_weighted else one(1200)])
    if rows_weighted and not base_weighted:
        # a unit base has dropped its duplicates: each of its EDGES counts 1 beside the weighted rows, so "the base's rows" are
        # its resident pairs; the masks of a typed one come from the restatement (the host constructor takes no masks)
        p0 = _host(base._pairs)
        want = _db().EntityGraph(N + 40, np.concatenate([p0, rows1]), weights=np.concatenate([one(len(p0)), w1]))
        assert np.array_equal(_host(got._pairs), _host(want._pairs)) and np.array_equal(_host(got._pair_weights), _host(want._pair_weights))
        ref = R.ingest_pairs(N + 40, rows1, w1, t1 if typed else None, base_pairs=p0, base_masks=_host(base._type_masks))
        assert np.array_equal(_host(got._pairs), ref.pairs) and np.array_equal(_host(got._pair_weights), ref.weights.astype(np.uint32))
        assert (ref.masks is None and got._type_masks is None) or np.array_equal(_host(got._type_masks), ref.masks)
    else:
        want = _db().EntityGraph(N + 40, np.concatenate([rows0, rows1]), weights=all_w, types=np.concatenate([t0, t1]) if typed else None)
        _same_graph(got, want)
        _same_answers(got, want, typed)
    assert got is not base and (base.n, np.array_equal(_host(base._pairs), before)) == (N, True)       # the receiver is not modified
    assert got.extended(np.zeros((0, 2), np.int64), types=np.zeros(0, np.int64) if typed else None).m == got.m


# ---- MentionMap ----------------------------------------------------------------------------------------------------------------------------
def _mention_rows(seed, n_chunks, n_entities, r):
    rng = np.random.default_rng(seed)
    rows = np.stack([rng.integers(0, n_chunks, r), rng.integers(0, n_entities, r)], axis=1).astype(np.int64)
    rows = np.concatenate([rows, np.stack([np.full(80, 5), np.arange(80)], axis=1)])                 # chunk 5 goes past the split degree
    return rows, rng.integers(1, 6, len(rows))


@pytest.mark.parametrize("weighted", [False, True])
def test_mention_maps_equal_the_host_constructor_and_rank_the_same_chunks(weighted):
    rows0, w0 = _mention_rows(4, 200, N, 2000)
    rows1, w1 = _mention_rows(5, 260, N + 40, 1500)
    w0, w1 = (w0, w1) if weighted else (None, None)
    want0 = _db().MentionMap(200, N, rows0, weights=w0)
    got0 = _db().MentionMap.from_rows(200, N, rows0, weights=w0)
    _same_map(got0, want0)
    assert got0.n_split >= 1 and got0.skipped == dict.fromkeys(R.MENTION_KINDS, 0)
    want1 = _db().MentionMap(260, N + 40, np.concatenate([rows0, rows1]), weights=None if w0 is None else np.concatenate([w0, w1]))
    got1 = got0.extended(rows1, weights=w1, n_chunks=260, n_entities=N + 40)
    _same_map(got1, want1)
    _same_map(got0, want0)                                              # the receiver is not modified
    _same_map(want0.extended(torch.from_numpy(rows1).cuda(), weights=None if w1 is None else torch.from_numpy(w1.astype(np.int32)).cuda(),
                             n_chunks=260, n_entities=N + 40), want1)
    grows, gw, _ = _rows(6, n=N + 40)
    graph = _db().EntityGraph(N + 40, grows, weights=gw)
    seeds = [[0, 5], [17], [330, 3]]
    assert np.array_equal(graph.rank_chunks(got1, seeds), graph.rank_chunks(want1, seeds))
    for x, y in zip(graph.rank_chunks(got1, seeds, top_k=15), graph.rank_chunks(want1, seeds, top_k=15)):
        assert np.array_equal(x, y)


# ---- RelationList.extended -------------------------------------------------------------------------------------------------------------------
def test_an_extended_relation_list_keeps_its_row_numbers():
    rows0, w0, t0 = _rows(7, r=800)
    rows1, w1, t1 = _rows(8, r=300)
    graph = _db().EntityGraph(N, np.concatenate([rows0, rows1]), types=np.concatenate([t0, t1]))
    rel0 = _db().RelationList(N, rows0, weights=w0.astype(np.float32), types=t0)
    rel1 = rel0.extended(rows1, weights=w1.astype(np.float32), types=t1)
    whole = _db().RelationList(N, np.concatenate([rows0, rows1]), weights=np.concatenate([w0, w1]).astype(np.float32), types=np.concatenate([t0, t1]))
    assert (rel1.r, rel0.r, rel1.n_entities) == (1100, 800, N) and rel1 is not rel0
    seeds = [[0, 5], [17]]
    a, b, old = (graph.subgraph(seeds, hops=2, relations=x) for x in (rel1, whole, rel0))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    typed = graph.subgraph(seeds, hops=2, relations=rel1, relation_types=[1, 2, 3]), graph.subgraph(seeds, hops=2, relations=whole, relation_types=[1, 2, 3])
    for x, y in zip(*typed):
        assert np.array_equal(x, y)
    for q in range(2):                                                  # the old table's rows are the new table's rows below 800
        ids = a.edge_ids[q, :a.edge_counts[q]]
        assert np.array_equal(ids[ids < 800], old.edge_ids[q, :old.edge_counts[q]]) and (ids >= 800).any()
    assert rel0.extended(rows1, weights=w1, types=t1, n_entities=N + 5).n_entities == N + 5


# ---- on_invalid --------------------------------------------------------------------------------------------------------------------------------
def test_on_invalid_raises_or_skips_and_reports():
    rows = [[0, 1], [1, 0], [5, 5], [0, N], [2, 3], [2, 3], [4, 6]]
    w, t = [1, 2, 1, 1, 0, 7, 1], [0, 1, 0, 0, 0, 2, 32]
    with pytest.raises(ValueError, match="out_of_range=1, self_loop=1, zero_weight=1, bad_type=1"):
        _db().EntityGraph.from_rows(N, rows, weights=w, types=t)
    g = _db().EntityGraph.from_rows(N, rows, weights=w, types=t, on_invalid="skip")
    assert g.skipped == {"out_of_range": 1, "self_loop": 1, "zero_weight": 1, "bad_type": 1}
    assert _host(g._pairs).tolist() == [[0, 1], [2, 3]] and _host(g._pair_weights).tolist() == [3, 7] and _host(g._type_masks).tolist() == [3, 4]
    with pytest.raises(ValueError, match="self_loop=1"):
        g.extended([[9, 9]], weights=[1], types=[0])
    assert g.extended([[9, 9], [7, 8]], weights=[1, 1], types=[0, 0], on_invalid="skip").m == 3
    mrows, mw = [[0, 0], [3, 0], [0, 9], [1, 1], [1, 2]], [1, 1, 1, 4096, 5]
    with pytest.raises(ValueError, match="chunk_out_of_range=1, entity_out_of_range=1, bad_weight=1"):
        _db().MentionMap.from_rows(3, 3, mrows, weights=mw)
    m = _db().MentionMap.from_rows(3, 3, mrows, weights=mw, on_invalid="skip")
    assert m.skipped == {"chunk_out_of_range": 1, "entity_out_of_range": 1, "bad_weight": 1} and m.nnz == 2
    with pytest.raises(ValueError, match="chunk_out_of_range=1"):
        m.extended([[3, 0]])
    assert m.extended([[3, 0]], n_chunks=4).n_chunks == 4


# ---- refusals: nothing is built ----------------------------------------------------------------------------------------------------------------
def test_refusals_from_the_devices_own_maxima():
    B = _B()
    top = (1 << 32) - 1
    with pytest.raises(B.RarcUnsupported, match="add up to 8589934590"):
        _db().EntityGraph.from_rows(5, [[0, 1], [1, 0]], weights=[top, top])
    with pytest.raises(B.RarcUnsupported, match="total edge weight"):
        _db().EntityGraph.from_rows(5, [[0, 1], [1, 2]], weights=[1 << 30, 1 << 30])
    base = _db().EntityGraph(5, [[0, 1]], weights=[(1 << 31) - 2])
    with pytest.raises(B.RarcUnsupported, match="total edge weight"):
        base.extended([[3, 4]], weights=[2])
    assert base.extended([[3, 4]]).m == 2                               # (a unit row beside a weighted base counts 1: the total is 2^31 - 1)
    assert _host(base.extended([[1, 0]], weights=[1])._pair_weights).tolist() == [(1 << 31) - 1]
    for rows in ([[1, 1]], [[0, 9]], np.zeros((0, 2), np.int64)):
        with pytest.raises(ValueError, match="at least 1 edge"):
            _db().EntityGraph.from_rows(5, rows, on_invalid="skip")
    with pytest.raises(B.RarcUnsupported, match="add up to 4096"):
        _db().MentionMap.from_rows(2, 2, [[0, 1], [0, 1]], weights=[4095, 1])
    m = _db().MentionMap(2, 2, [[0, 1]], weights=[4000])
    with pytest.raises(B.RarcUnsupported, match="add up to 4096"):
        m.extended([[0, 1]], weights=[96])
    assert _host(m.extended([[0, 1]], weights=[95])._w).tolist() == [4095]
    for rows in ([[5, 0]], np.zeros((0, 2), np.int64)):
        with pytest.raises(ValueError, match="at least 1 mention"):
            _db().MentionMap.from_rows(2, 2, rows, on_invalid="skip")
    with pytest.raises(ValueError, match="the graph carries relation types"):
        _db().EntityGraph(5, [[0, 1]], types=[3]).extended([[1, 2]])
    with pytest.raises(ValueError, match="smaller than the graph's"):
        base.extended([[1, 2]], n=4)
    damaged = _db().EntityGraph(5, [[0, 1], [1, 2]])
    damaged._pairs = torch.tensor([[0, 1], [2, 1]], dtype=torch.int64, device="cuda")
    with pytest.raises(B.RarcError, match="damaged"):
        damaged.extended([[3, 4]])


# ---- add_documents -------------------------------------------------------------------------------------------------------------------------------
def _corpus():
    from tests import passage_ref as P
    from tests.helpers import HashEmbeddings

    n_ent, n_chunks = 48, 36
    emb = HashEmbeddings(64)
    x = np.asarray(emb.embed_documents([f"entity {i}" for i in range(n_ent)]), np.float32)
    chunks, ids = [f"chunk {i} of the corpus" for i in range(n_chunks)], [f"c{i}" for i in range(n_chunks)]
    mentions, mw = P.random_mentions(n_ent, n_chunks, seed=31, max_degree=4, max_weight=9)
    mentions = np.asarray(mentions, np.int64).reshape(-1, 2)
    pairs, pw, pt = _rows(32, n=n_ent, r=160)
    return emb, x, chunks, ids, mentions, np.asarray(mw), pairs, pw, pt


QUERIES = ["entity 3", "entity 41", "who founded entity 5", "an unrelated question", "entity 30 and entity 44"]


def _answers(r, **kw):
    return [[(d.id, d.content, d.score) for d in docs] for docs in r.batch_invoke(QUERIES, k=6, **kw)]


@pytest.mark.parametrize("form", ["pairs", "typed_k_hop", "cooccurrence"])
def test_add_documents_equals_a_retriever_built_from_everything_at_once(form):
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    emb, x, chunks, ids, mentions, mw, pairs, pw, pt = _corpus()
    e0, c0 = 40, 28                                                     # the first batch: 40 entities, 28 chunks
    old_m = (mentions[:, 0] < c0) & (mentions[:, 1] < e0)
    old_p = (pairs < e0).all(axis=1)
    kw = {"k": 5}
    if form == "typed_k_hop":
        kw.update(expansion="k_hop", hops=2, relation_types=list(range(20)))
    graph_kw = lambda keep: {} if form == "cooccurrence" else dict(                                  # noqa: E731
        pairs=pairs[keep], pair_weights=pw[keep], **({"pair_types": pt[keep]} if form == "typed_k_hop" else {}))
    whole = HipGraphRetriever.from_arrays(emb, x, mentions=mentions, texts=chunks, mention_weights=mw, ids=ids, **graph_kw(slice(None)), **kw)
    grown = HipGraphRetriever.from_arrays(emb, x[:e0], mentions=mentions[old_m], texts=chunks[:c0], mention_weights=mw[old_m], ids=ids[:c0],
                                          **graph_kw(old_p), **kw)
    before, old_graph, old_map = _answers(grown), grown.graph, grown.mentions
    # a failing call — a mention names a chunk that does not exist — changes nothing
    with pytest.raises(ValueError, match="chunk_out_of_range=1"):
        grown.add_documents(chunks[c0:], np.concatenate([mentions[~old_m], [[len(chunks), 0]]]), mention_weights=np.concatenate([mw[~old_m], [1]]),
                            entity_embeddings=x[e0:], ids=ids[c0:], **graph_kw(~old_p))
    assert grown.graph is old_graph and grown.mentions is old_map and len(grown.docs) == c0 and int(grown.index.ntotal) == e0
    assert _answers(grown) == before
    if form == "cooccurrence":
        with pytest.raises(ValueError, match="co-occurrence"):
            grown.add_documents(chunks[c0:], mentions[~old_m], mention_weights=mw[~old_m], entity_embeddings=x[e0:], pairs=pairs[~old_p])
        assert _answers(grown) == before
    assert grown.add_documents(chunks[c0:], mentions[~old_m], mention_weights=mw[~old_m], entity_embeddings=x[e0:], ids=ids[c0:],
                               **graph_kw(~old_p)) == ids[c0:]
    assert grown.graph is not old_graph and grown.get_document_count() == len(chunks) and int(grown.index.ntotal) == len(x)
    _same_graph(grown.graph, whole.graph)
    _same_map(grown.mentions, whole.mentions)
    got, want = _answers(grown), _answers(whole)
    assert got == want and any(len(a) for a in got) and got != before
