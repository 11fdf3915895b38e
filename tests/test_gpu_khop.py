"""EntityGraph.neighbourhood / expand / neighbourhood_chunks / expand_chunks on the GPU (csrc/khop.hip) against the restatement
tests/khop_ref.py: levels, counts, lists and chunk scores are equal element for element — the rule is ORs and integer sums, so
there is no band; chunk scores are compared as float64 bits.  The shapes are the smallest that reach each path: one word per
vertex and two, three and four, a partial last word, a vertex one above the degree at which it is split across a workgroup and
one of several rounds of it, more than one tile of the list, a chunk of more than 64 mentions, and n a multiple of no tile."""
import numpy as np
import pytest

from tests import khop_ref as K
from tests import passage_ref as P
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu


def _graph(n, edges):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, edges)


def _map(n_chunks, n, mentions, weights=None):
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    return MentionMap(n_chunks, n, mentions, weights=weights)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(g, n, edges, seeds, hops, caps=(), lv=None, **kw):
    """dense levels, then for every cap: ids, hops, counts and hop_counts -> the reference levels"""
    lv = K.levels(n, edges, seeds, hops) if lv is None else lv
    got = g.neighbourhood(seeds, hops=hops, **kw)
    assert got.dtype == np.uint8 and got.shape == lv.shape
    assert np.array_equal(got, lv), np.argwhere(got != lv)[:5]
    for cap in caps:
        ids, hp, cnt, hc = g.neighbourhood(seeds, hops=hops, max_vertices=cap, **kw)
        assert (ids.dtype, hp.dtype, cnt.dtype, hc.dtype) == (np.int64, np.int32, np.int32, np.int32)
        wi, wh, wc = K.listing(lv, cap)
        assert np.array_equal(hc, K.counts(lv, hops)), cap
        assert np.array_equal(cnt, wc) and np.array_equal(ids, wi) and np.array_equal(hp, wh), cap
    return lv


# ---- small graphs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [0, 1, 3, 8])
def test_a_path_from_an_end_and_from_the_middle(hops):
    n, edges = 20, K.path_graph(20)
    lv = _check(_graph(n, edges), n, edges, [[0], [10], [19, 0], [10, 11]], hops, caps=(1, 5, 20, 30))
    assert lv[0, :hops + 1].tolist() == list(range(hops + 1)) and np.all(lv[0, hops + 1:] == 255)
    assert (lv[1] != 255).sum() == 2 * hops + 1                                    # 10 - 8 .. 10 + 8 stay inside the path


@pytest.mark.parametrize("rounds", [1, 4])
def test_a_hub_of_more_neighbours_than_a_group_walks(rounds):
    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood

    split = neighbourhood.limits()["split_degree"]
    leaves = split + 1 if rounds == 1 else 4 * split + 3
    n, edges = K.star_graph(leaves)
    edges = edges + [(leaves, n)]                                                  # a tail behind the last leaf: the hub is a way through
    g = _graph(n + 1, edges)
    for hops in (1, 2, 3):
        lv = _check(g, n + 1, edges, [[1], [0], [n], [1, leaves]], hops, caps=(1, leaves, n + 1))
        assert lv[0, 0] == 1 and lv[1, 0] == 0 and (lv[0, 2] == 2 if hops >= 2 else lv[0, 2] == 255)
    # the same hub without its edge to the leaf the seed sits on, at the split degree exactly: the group form walks it
    n2, e2 = K.star_graph(split)
    _check(_graph(n2, e2), n2, e2, [[1], [0]], 2, caps=(n2,))


def test_two_vertices():
    g = _graph(2, [(0, 1)])
    for hops in (0, 1, 8):
        _check(g, 2, [(0, 1)], [[0], [1], [0, 1], []], hops, caps=(1, 2, 3))


def test_two_components_isolated_vertices_and_a_seed_on_one():
    n, edges = K.two_components_and_isolated()
    n += 3                                                                         # vertices above the largest any pair names
    g = _graph(n, edges)
    for hops in (0, 1, 2, 8):
        lv = _check(g, n, edges, [[0], [6], [10], [n - 1], [0, 9, 11]], hops, caps=(1, 4, n))
        assert (lv[2] != 255).sum() == 1 and (lv[3] != 255).sum() == 1 and np.all(lv[0, 6:] == 255)


def test_no_seeds_unused_slots_and_a_repeated_seed():
    import torch

    n, edges = 50, K.random_graph(50, 80, 3)[0]
    g = _graph(n, edges)
    lv = _check(g, n, edges, [[], [7, 7, 7], [7], [3, 7, 3]], 2, caps=(1, n))
    assert np.all(lv[0] == 255) and np.array_equal(lv[1], lv[2])
    slots = torch.tensor([[-1, -1, -1], [-1, 7, -1], [7, 7, 7], [-1, -1, 4]], dtype=torch.int64, device="cuda")
    want = K.levels(n, edges, [[], [7], [7], [4]], 2)
    assert np.array_equal(g.neighbourhood(slots, hops=2), want)
    ids, hp, cnt, hc = g.neighbourhood(slots, hops=2, max_vertices=4)
    assert cnt[0] == 0 and np.all(ids[0] == -1) and np.all(hp[0] == -1) and np.all(hc[0] == 0)
    with pytest.raises(ValueError):
        g.neighbourhood([[n]])
    with pytest.raises(ValueError):
        g.neighbourhood([list(range(40)) + list(range(25))])
    with pytest.raises(ValueError):
        g.neighbourhood([[0]], hops=-1)


# ---- the random graph: n is a multiple of no tile size ---------------------------------------------------------------------------------
N, M = 5003, 20011
ALL_HOPS = (0, 1, 2, 3, 8)
SLOTS = (1, 5, 64)


@pytest.fixture(scope="module")
def world():
    """the graph, and per n_slots 256 seed rows with their reference levels at 8 hops, computed once and shared"""
    edges, _ = K.random_graph(N, M, seed=31)
    seeds = {s: K.random_seeds(N, 256, s, seed=40 + s) for s in SLOTS}
    lv8 = {s: K.levels(N, edges, seeds[s], 8) for s in SLOTS}
    for lv in lv8.values():
        lv.setflags(write=False)
    return {"edges": edges, "g": _graph(N, edges), "seeds": seeds, "lv8": lv8}


def _cut(lv8, hops):
    """the levels at fewer hops (tests/test_khop_ref_host.py holds levels() to the definition at every hops)"""
    return np.where(lv8 <= hops, lv8, K.NOT_WITHIN).astype(np.uint8)


def test_the_shared_reference_cut_at_fewer_hops_is_the_reference_at_fewer_hops(world):
    for hops in (0, 2):
        assert np.array_equal(_cut(world["lv8"][5][:9], hops), K.levels(N, world["edges"], world["seeds"][5][:9], hops))


@pytest.mark.parametrize("nq", [1, 2, 63, 64, 65, 128, 255, 256])
@pytest.mark.parametrize("n_slots", SLOTS)
def test_random_graph_levels_counts_and_lists(world, nq, n_slots):
    for hops in ALL_HOPS:
        lv = _cut(world["lv8"][n_slots][:nq], hops)
        _check(world["g"], N, world["edges"], world["seeds"][n_slots][:nq], hops, caps=(300,), lv=lv)
    assert (world["lv8"][n_slots][:nq] != 255).any()


def test_row_q_of_a_batch_equals_the_one_query_call_and_batches_above_256_are_cut(world):
    g, seeds = world["g"], world["seeds"][5]
    batch = g.neighbourhood(seeds[:130], hops=3)
    bl = g.neighbourhood(seeds[:130], hops=3, max_vertices=200)
    for q in (0, 1, 63, 64, 65, 129):
        assert np.array_equal(g.neighbourhood([seeds[q]], hops=3)[0], batch[q])
        one = g.neighbourhood([seeds[q]], hops=3, max_vertices=200)
        assert all(np.array_equal(a[0], b[q]) for a, b in zip(one, bl))
    many = seeds + seeds[:44]
    got = g.neighbourhood(many, hops=2)
    assert got.shape == (300, N) and np.array_equal(got[:256], _cut(world["lv8"][5], 2)) and np.array_equal(got[256:], got[:44])
    ids, hp, cnt, hc = g.neighbourhood(many, hops=2, max_vertices=50)
    assert ids.shape == (300, 50) and hc.shape == (300, 3) and np.array_equal(ids[256:], ids[:44]) and np.array_equal(hc[256:], hc[:44])


def test_the_answer_does_not_depend_on_the_order_of_the_pairs_or_on_where_they_live(world):
    import torch

    edges, seeds = world["edges"], world["seeds"][5][:70]
    want = _cut(world["lv8"][5][:70], 3)
    rng = np.random.default_rng(5)
    shuffled = [edges[i] if rng.random() < 0.5 else (edges[i][1], edges[i][0]) for i in rng.permutation(len(edges))]
    assert np.array_equal(_graph(N, shuffled).neighbourhood(seeds, hops=3), want)
    on_device = torch.tensor(sorted(edges), dtype=torch.int64, device="cuda")
    g = _graph(N, on_device)
    assert np.array_equal(g.neighbourhood(seeds, hops=3), want)
    dev = g.neighbourhood(seeds, hops=3, as_device=True)
    assert dev.is_cuda and dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), want)


def test_the_cap_cuts_the_list_in_order_and_leaves_the_counts(world):
    g, seeds = world["g"], world["seeds"][5][:3]
    lv = _cut(world["lv8"][5][:3], 3)
    hc = K.counts(lv, 3)
    size = int(hc[0].sum())
    assert size > 1200 and hc[0, 2] > 4                                           # (more than one tile of the list holds entries)
    caps = (size, size - 1, int(hc[0, :2].sum()) + int(hc[0, 2]) // 2, int(hc[0, :2].sum()), 1)
    _check(g, N, world["edges"], seeds, 3, caps=caps, lv=lv)
    from rag_arc_amd.hip.binding import RarcUnsupported

    with pytest.raises(RarcUnsupported, match="65536"):
        g.neighbourhood(seeds, hops=3, max_vertices=65537)
    with pytest.raises(RarcUnsupported, match="8"):
        g.neighbourhood(seeds, hops=9)
    ids, hp, cnt, _ = g.neighbourhood(seeds, hops=1, max_vertices=65536)
    assert ids.shape == (3, 65536) and np.array_equal(cnt, K.counts(lv, 1).sum(axis=1)) and np.all(ids[0, cnt[0]:] == -1)


def _stepwise(g, seeds, hops, stop_when_idle):
    """the entry points one by one -> (levels, the grew word after every step taken)"""
    import torch

    from rag_arc_amd.encapsulation.database.graph_db import neighbourhood as KH
    from rag_arc_amd.hip import binding as B

    lib, n, m = g.lib, g.n, g.m
    sd = torch.from_numpy(KH.host_seeds(n, seeds)).cuda()
    nq = int(sd.shape[0])
    ws = torch.empty(int(lib.rarc_khop_workspace_bytes(n, m, nq, hops)), dtype=torch.uint8, device="cuda")
    grew = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    B.check(lib.rarc_khop_seed(n, m, sd.data_ptr(), nq, int(sd.shape[1]), hops, ws.data_ptr(), ws.numel(), None), "seed")
    words = []
    for hop in range(1, hops + 1):
        B.check(lib.rarc_khop_step(g._graph.data_ptr(), g._graph.numel(), n, m, nq, hops, hop, ws.data_ptr(), ws.numel(), grew.data_ptr(), None),
                "step")
        words.append(int(grew.item()))
        if stop_when_idle and not words[-1]:
            break
    out = torch.empty((nq, n), dtype=torch.uint8, device="cuda")
    B.check(lib.rarc_khop_levels(n, m, nq, hops, ws.data_ptr(), ws.numel(), out.data_ptr(), None), "levels")
    return out.cpu().numpy(), words


def test_early_stop_on_a_graph_of_diameter_3():
    edges = [(0, 1), (1, 2), (2, 3)] + [(1, v) for v in range(4, 40)] + [(2, v) for v in range(40, 90)]
    n = 92                                                                         # 90 and 91 are isolated
    assert K.levels(n, edges, [[0]], 8).max() == 255 and K.levels(n, edges, [[0]], 8)[0, :90].max() == 3
    g = _graph(n, edges)
    seeds = [[0], [3], [1, 90], []]
    want = K.levels(n, edges, seeds, 8)
    assert np.array_equal(g.neighbourhood(seeds, hops=8, early_stop=True), want)
    assert np.array_equal(g.neighbourhood(seeds, hops=8, early_stop=False), want)
    for a, b in zip(g.neighbourhood(seeds, hops=8, max_vertices=n, early_stop=True), g.neighbourhood(seeds, hops=8, max_vertices=n)):
        assert np.array_equal(a, b)
    stopped, w1 = _stepwise(g, seeds, 8, True)
    full, w2 = _stepwise(g, seeds, 8, False)
    assert np.array_equal(stopped, want) and np.array_equal(full, want)
    assert w1 == [1, 1, 1, 0] and w2 == [1, 1, 1, 0, 0, 0, 0, 0]                  # 0 from the first empty level on


# ---- chunks ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passages():
    n, n_chunks = 400, 301
    edges, _ = K.random_graph(n, 700, seed=51)
    mentions, weights = P.random_mentions(n, n_chunks - 1, seed=52, max_degree=9, max_weight=30)
    big, big_w = P.chunk_of_degree(n, 150, seed=53, chunk=n_chunks - 1, max_weight=20)      # one chunk of more than 64 mentions
    mentions, weights = mentions + big, weights + big_w
    assert len({c for c, _ in mentions}) < n_chunks                                # chunks without mentions
    return {"n": n, "n_chunks": n_chunks, "edges": edges, "mentions": mentions, "weights": weights, "g": _graph(n, edges),
            "mm": _map(n_chunks, n, mentions, weights), "seeds": K.random_seeds(n, 70, 3, seed=54) + [[]]}


@pytest.mark.parametrize("hops,decay", [(2, None), (0, None), (3, [100, 0, 65536, 1]), (8, None), (1, [0, 0])])
def test_chunk_scores_and_their_top_k(passages, hops, decay):
    f = passages
    lv = K.levels(f["n"], f["edges"], f["seeds"], hops)
    table = K.default_decay(hops) if decay is None else decay
    want = K.chunk_scores(lv, f["n_chunks"], f["mentions"], f["weights"], table)
    for seeds in (f["seeds"], f["seeds"][:1], f["seeds"][:64]):
        got = f["g"].neighbourhood_chunks(f["mm"], seeds, hops=hops, decay=decay)
        assert got.dtype == np.float64 and got.shape == (len(seeds), f["n_chunks"])
        assert np.array_equal(_bits(got), _bits(want[:len(seeds)]))
    assert (want[:, -1] > 0).any() or decay == [0, 0]                              # the split chunk scores
    for k in (1, 10, f["n_chunks"]):
        ids, sc, cnt = f["g"].neighbourhood_chunks(f["mm"], f["seeds"], hops=hops, decay=decay, top_k=k)
        for q in range(len(f["seeds"])):
            S = [int(x) for x in np.rint(want[q] * K.SCORE_ONE)]
            wi, wsc, wc = K.chunk_topk(S, k)
            assert cnt[q] == wc and ids[q].tolist() == wi and _bits(sc[q]).tolist() == _bits(wsc).tolist(), (k, q)
            assert all(s > 0 for s in sc[q, :cnt[q]])                              # a chunk of score 0 is never returned


def test_a_chunk_of_more_than_64_mentions_that_the_split_list_omits_scores_0(passages):
    f = passages
    mm = _map(f["n_chunks"], f["n"], f["mentions"], f["weights"])
    assert mm.n_split == 1
    mm._split, mm.n_split = None, 0
    lv = K.levels(f["n"], f["edges"], f["seeds"], 2)
    want = K.chunk_scores(lv, f["n_chunks"], f["mentions"], f["weights"], K.default_decay(2))
    assert (want[:, -1] > 0).any()
    want[:, -1] = 0.0
    assert np.array_equal(_bits(f["g"].neighbourhood_chunks(mm, f["seeds"], hops=2)), _bits(want))


def test_chunk_arguments(passages):
    f = passages
    for decay in ([1, 2], [1, 2, 65537], [1, 2, -1]):
        with pytest.raises(ValueError, match="decay"):
            f["g"].neighbourhood_chunks(f["mm"], f["seeds"], hops=2, decay=decay)
    with pytest.raises(ValueError):
        f["g"].neighbourhood_chunks(object(), f["seeds"])
    with pytest.raises(ValueError):
        f["g"].neighbourhood_chunks(_map(5, f["n"] + 1, [(0, 1)]), f["seeds"])


# ---- seeds from the index, and the retriever --------------------------------------------------------------------------------------------
N_ENT, N_CHUNKS, DIM = 2000, 300, 64
QUERIES = ["entity 3", "entity 1717", "who founded entity 5", "entity 1999", "an unrelated question"]


@pytest.fixture(scope="module")
def indexed():
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    emb = HashEmbeddings(DIM)
    x = np.asarray(emb.embed_documents([f"entity {i}" for i in range(N_ENT)]), np.float32)
    edges, _ = K.random_graph(N_ENT, 3000, seed=61)
    mentions, weights = P.random_mentions(N_ENT, N_CHUNKS, seed=62, max_degree=8, max_weight=9)
    texts, ids = [f"chunk {i} of the corpus" for i in range(N_CHUNKS)], [f"c{i}" for i in range(N_CHUNKS)]
    r = HipGraphRetriever.from_arrays(emb, x, edges, mentions, texts, mention_weights=weights, ids=ids, k=5, expansion="k_hop", hops=2)
    q = np.asarray([emb.embed_query(t) for t in QUERIES], np.float32)
    return {"emb": emb, "x": x, "edges": edges, "mentions": mentions, "weights": weights, "texts": texts, "ids": ids, "r": r, "q": q}


def test_expand_takes_the_seeds_the_index_search_returns(indexed):
    f, r = indexed, indexed["r"]
    _, I = r.index.search(f["q"], 5)
    seeds = [row.tolist() for row in I]
    for hops in (1, 2):
        assert np.array_equal(r.graph.expand(r.index, f["q"], seeds_per_query=5, hops=hops), r.graph.neighbourhood(seeds, hops=hops))
        assert np.array_equal(r.graph.neighbourhood(seeds, hops=hops), K.levels(N_ENT, f["edges"], seeds, hops))
        a = r.graph.expand(r.index, f["q"], seeds_per_query=5, hops=hops, max_vertices=64)
        b = r.graph.neighbourhood(seeds, hops=hops, max_vertices=64)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        got = r.graph.expand_chunks(r.index, f["q"], r.mentions, seeds_per_query=5, hops=hops, top_k=12)
        want = r.graph.neighbourhood_chunks(r.mentions, seeds, hops=hops, top_k=12)
        assert all(np.array_equal(x, y) for x, y in zip(got, want)) and got[2].min() > 0
    with pytest.raises(ValueError):
        r.graph.expand(r.index, f["q"], seeds_per_query=65)


def test_the_retriever_returns_the_documents_in_the_reference_order(indexed):
    f, r = indexed, indexed["r"]
    _, I = r.index.search(f["q"], 5)
    lv = K.levels(N_ENT, f["edges"], [row.tolist() for row in I], 2)
    want = K.chunk_scores(lv, N_CHUNKS, f["mentions"], f["weights"], K.default_decay(2))
    batch = r.batch_invoke(QUERIES, k=7)
    for i, text in enumerate(QUERIES):
        wi, wsc, wc = K.chunk_topk([int(x) for x in np.rint(want[i] * K.SCORE_ONE)], 7)
        docs = r.invoke(text, k=7)
        assert [d.id for d in docs] == [f["ids"][c] for c in wi[:wc]] and [d.score for d in docs] == wsc[:wc] and wc > 0
        assert [d.content for d in docs] == [f["texts"][c] for c in wi[:wc]]
        assert [(d.id, d.content, d.score) for d in batch[i]] == [(d.id, d.content, d.score) for d in docs]
    assert len(r.invoke(QUERIES[0])) == 5 and r.batch_invoke([]) == [] and not hasattr(r.docs[0], "score")


def test_the_registered_config_builds_the_k_hop_retriever_and_an_unknown_expansion_raises(indexed, tmp_path):
    import json

    from rag_arc_amd.config.app_registration import register_graph_retriever, registrator
    from rag_arc_amd.core.retrieval import HipGraphRetriever

    f, r = indexed, indexed["r"]
    np.savez(tmp_path / "graph.npz", pairs=np.asarray(f["edges"], np.int64), mentions=np.asarray(f["mentions"], np.int64),
             mention_weights=np.asarray(f["weights"], np.int64), entity_embeddings=f["x"], texts=np.array(f["texts"]), ids=np.array(f["ids"]))
    np.savez(tmp_path / "emb.npz", texts=np.array(QUERIES), vectors=f["q"])
    cfg = {"type": "hip_graph_retriever", "graph_path": str(tmp_path / "graph.npz"), "k": 5, "expansion": "k_hop", "hops": 3, "decay": [9, 3, 1, 0],
           "embedding": {"type": "table_embeddings", "path": str(tmp_path / "emb.npz")}}
    (tmp_path / "graph.json").write_text(json.dumps(cfg))
    register_graph_retriever(str(tmp_path / "graph.json"), "t_khop_retriever")
    app = registrator.get_object("t_khop_retriever")
    assert (app.expansion, app.hops, app.decay.tolist()) == ("k_hop", 3, [9, 3, 1, 0])
    ids, sc, cnt = r.graph.expand_chunks(r.index, f["q"], r.mentions, seeds_per_query=5, hops=3, decay=[9, 3, 1, 0], top_k=8)
    for i, text in enumerate(QUERIES):
        got = app.invoke(text, k=8)
        assert [d.id for d in got] == [f["ids"][c] for c in ids[i, :cnt[i]]] and [d.score for d in got] == sc[i, :cnt[i]].tolist() and got
    default = HipGraphRetriever(r.embedding, r.index, r.graph, r.mentions, r.docs)
    assert default.expansion == "ppr" and [d.id for d in default.invoke(QUERIES[0])] != [] and default.decay is None
    for bad in ("bfs", "", None):
        with pytest.raises(ValueError, match="expansion"):
            HipGraphRetriever(r.embedding, r.index, r.graph, r.mentions, r.docs, expansion=bad)
    with pytest.raises(ValueError, match="decay"):
        HipGraphRetriever(r.embedding, r.index, r.graph, r.mentions, r.docs, expansion="k_hop", hops=2, decay=[1, 2])
