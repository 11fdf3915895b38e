"""Filtered search with one filter PER QUERY on the GPU: FlatIndexF16.search_filtered_many (csrc/subset.hip:
rarc_search_rows_grouped, rarc_strike_rows_grouped) and the store's `filters=` / its coalescing front under `filter=`.

The reference is tests/subset_ref.search PER QUERY over that query's own allowed rows — ids AND score bits — never
search_filtered.  One master list of 264 queries over n = 70,001 rows of 128 dimensions carries 39 groups whose lists hold
0, 1, 31, 33, 5000, 32768, 32769 and 70,001 rows (with 256 queries in the row-list search a slab is 32768 rows: no round, one,
exactly one, one plus one row, three rounds — in the same call), 1, 7, 8 or 9 queries per group (the tile edges at 8 queries
per tile), groups interleaved in caller order, unfiltered (None) entries among them.  The smaller calls (40 queries, one
query) answer positions of the same list, so one reference per (storage, metric), computed once at k = 100 and left
unchanged, serves all of them: the reference's answer for a smaller k is its prefix.  Twenty rows are copies of twenty others
and the first query of every group IS one of them: equal scores, decided by id, at the top of its answer."""
import threading

import numpy as np
import pytest

from tests import l2_ref, subset_ref
from tests.helpers import HashEmbeddings

pytestmark = pytest.mark.gpu

N, D = 70_001, 128
SIZES = [0, 1, 31, 33, 5000, 32768, 32769, 70_001]
COUNTS = [1, 7, 8, 9]
K_REF = 100


@pytest.fixture(scope="module")
def hip():
    import torch

    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from rag_arc_amd.hip import engine

    return engine


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_MASTER: dict = {}


def _master():
    """Rows, queries and the per-query allowed rows of the master list; made once, left unchanged."""
    if not _MASTER:
        rng = np.random.default_rng(4100)
        X = rng.standard_normal((N, D)).astype(np.float32)
        src = np.arange(100, 120)
        dst = rng.choice(np.arange(1000, N), 20, replace=False)
        X[dst] = X[src]                                  # twenty copies at other positions: equal scores, the id decides
        pairs = np.stack([src, dst], axis=1).reshape(-1)
        groups = [(m, c) for m in SIZES for c in COUNTS] + [(33, 8)] * 7           # 200 + 56 = 256 filtered queries
        allowed = []
        for m, _ in groups:
            if m == N:
                a = np.arange(N)
            elif m == 1:
                a = np.array([dst[0]])
            else:
                forced = pairs[: min(m, 6)]              # (src0, dst0), (src1, dst1), (src2, dst2) as far as they fit
                rest = np.setdiff1d(np.arange(N), pairs)
                a = np.sort(np.concatenate([forced, rng.choice(rest, m - forced.size, replace=False)]))
            allowed.append(a.astype(np.int64))
        order = rng.permutation(np.repeat(np.arange(len(groups)), [c for _, c in groups]))      # groups interleaved
        big = [g for g, (m, c) in enumerate(groups) if c == 1]                                   # one-query groups, every m
        tail = [big[4], None, big[7], None, big[0], None, None, big[5]]                          # [a, None, b, None, ...]
        which = list(order) + tail
        Q = rng.standard_normal((len(which), D)).astype(np.float32)
        seen = set()
        for i, g in enumerate(which):                    # the first query of a group is row src[0] itself
            if g is not None and g not in seen:
                seen.add(g)
                Q[i] = X[src[0]]
        _MASTER.update(X=X, Q=Q, groups=groups, allowed=allowed, which=which, src=src, dst=dst)
    return _MASTER


_INDEX: dict = {}
_REF: dict = {}


def _index(hip, storage, metric):
    """One index per (storage, metric) with one RowSet per group of the master list (and the list of RowSets per query)."""
    if (storage, metric) not in _INDEX:
        M = _master()
        idx = hip.FlatIndexF16(D, metric=metric, storage=storage)
        idx.add(M["X"])
        sets = [idx.rowset(a) for a in M["allowed"]]
        _INDEX[(storage, metric)] = (idx, sets, [None if g is None else sets[g] for g in M["which"]])
    return _INDEX[(storage, metric)]


def _reference(oracle, storage, metric):
    """(D [264][100], I [264][100]): subset_ref.search of every query of the master list over its own allowed rows."""
    if (storage, metric) not in _REF:
        M = _master()
        normalize = metric == "cosine"
        rows = l2_ref.stored_rows(oracle, M["X"], storage, normalize)
        nq = len(M["which"])
        Dr, Ir = np.empty((nq, K_REF), np.float32), np.empty((nq, K_REF), np.int64)
        by_group: dict = {}
        for i, g in enumerate(M["which"]):
            by_group.setdefault(g, []).append(i)
        for g, pos in by_group.items():
            # subset_ref.search scores EVERY row it is given before it looks at the allowed ones (metric "l2" also takes every
            # row's norm, per call): it is given the group's allowed rows and nothing else, all of them allowed.  A row's
            # score does not depend on the rows around it, and position in the ascending list orders as the row number does
            # (the id tie-break), so the answer is the same with the ids mapped back.
            a = np.arange(N) if g is None else M["allowed"][g]
            Dg, Ig = subset_ref.search(oracle, rows[a], M["Q"][pos], K_REF, np.arange(a.size), "l2" if metric == "l2" else "ip", normalize)
            Dr[pos], Ir[pos] = Dg, np.where(Ig >= 0, a[np.maximum(Ig, 0)] if a.size else -1, -1)
        Dr.setflags(write=False)
        Ir.setflags(write=False)
        _REF[(storage, metric)] = (Dr, Ir)
    return _REF[(storage, metric)]


def _check(got, ref, pos, k, what):
    D_got, I_got = got
    D_ref, I_ref = ref[0][pos][:, :k], ref[1][pos][:, :k]
    assert D_got.shape == (len(pos), k) and I_got.shape == (len(pos), k), what
    bad = [int(pos[i]) for i in range(len(pos)) if not (np.array_equal(I_got[i], I_ref[i]) and np.array_equal(_bits(D_got[i]), _bits(D_ref[i])))]
    assert not bad, (what, "master positions that differ:", bad[:10])


@pytest.mark.parametrize("storage,metric", [("f16", "cosine"), ("f16", "ip"), ("f16", "l2"), ("f32", "cosine"), ("f32", "ip"), ("f32", "l2")])
def test_every_query_gets_the_answer_of_its_own_filter(hip, oracle, storage, metric):
    M = _master()
    idx, sets, per_query = _index(hip, storage, metric)
    ref = _reference(oracle, storage, metric)
    pos = np.arange(len(per_query))
    for k in (1, 10, 100):
        for strategy in ("subset", "overfetch", "auto"):
            got = idx.search_filtered_many(M["Q"], k, per_query, strategy=strategy)
            _check(got, ref, pos, k, (storage, metric, k, strategy))
    # padding beyond min(k, m): (-1, -inf) / metric "l2" (-1, +inf); the copies come out together, the smaller id first
    Dg, Ig = idx.search_filtered_many(M["Q"], 10, per_query)
    for i, g in enumerate(M["which"]):
        m = N if g is None else M["groups"][g][0]
        kk = min(10, m)
        assert (Ig[i, kk:] == -1).all() and (np.isposinf(Dg[i, kk:]) if metric == "l2" else np.isneginf(Dg[i, kk:])).all()
        assert g is None or np.isin(Ig[i, :kk], M["allowed"][g]).all()
    first = M["which"].index(next(g for g, (m, c) in enumerate(M["groups"]) if m == 5000 and c == 9))
    assert Ig[first, :2].tolist() == [int(M["src"][0]), int(M["dst"][0])] and _bits(Dg[first, 0]) == _bits(Dg[first, 1])


@pytest.mark.parametrize("storage,metric", [("f16", "cosine"), ("f32", "l2")])
def test_forty_queries_single_round_and_one_query(hip, oracle, storage, metric):
    """40 queries: a slab is 209 k rows, every group has a single round.  One query: the one-query kernel form."""
    M = _master()
    idx, sets, per_query = _index(hip, storage, metric)
    ref = _reference(oracle, storage, metric)
    want = [(5000, 7), (32769, 9), (70_001, 8), (0, 1), (33, 9), (1, 1), (31, 1)]
    gids = [M["groups"].index(w) for w in want]
    pos = [i for i, g in enumerate(M["which"][:256]) if g in gids] + [i for i, g in enumerate(M["which"]) if g is None]
    pos = np.array(sorted(pos))                           # caller order of the master list: interleaved
    assert len(pos) == 40 and sum(per_query[i] is None for i in pos) == 4
    for strategy in ("subset", "overfetch", "auto"):
        got = idx.search_filtered_many(M["Q"][pos], 10, [per_query[i] for i in pos], strategy=strategy)
        _check(got, ref, pos, 10, (storage, metric, strategy, "nq=40"))
    for g in (gids[1], gids[3], gids[0]):
        one = np.array([M["which"].index(g)])
        for strategy in ("subset", "overfetch", "auto"):
            ids, sc = idx.search_filtered_many_device(M["Q"][one], 10, [per_query[one[0]]], strategy=strategy)
            assert ids.is_cuda
            _check((sc.cpu().numpy(), ids.cpu().numpy()), ref, one, 10, (storage, metric, strategy, "nq=1"))
    one = np.array([M["which"].index(None)])
    _check(idx.search_filtered_many(M["Q"][one], 10, [None]), ref, one, 10, "nq=1 unfiltered")


def test_grouped_counters_and_more_than_256_queries(hip, oracle):
    M = _master()
    idx, sets, per_query = _index(hip, "f16", "cosine")
    before = dict(idx.filtered_stats)
    idx.search_filtered_many(M["Q"], 10, per_query, strategy="subset")
    after = idx.filtered_stats
    assert after["grouped_calls"] == before["grouped_calls"] + 1
    # two batches (256 + 8): 39 distinct RowSets in the first, 4 in the second
    assert after["groups"] == before["groups"] + 39 + 4
    assert after["subset_batches"] == before["subset_batches"] + 2 and after["fallback_queries"] == before["fallback_queries"]
    assert after["overfetch_batches"] == before["overfetch_batches"] + 1          # the None entries of the second batch


def test_wide_rows_take_four_queries_per_tile(hip, oracle):
    n, d = 3000, 2304
    rng = np.random.default_rng(77)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[2000:2004] = X[5]
    Q = rng.standard_normal((8, d)).astype(np.float32)
    Q[0] = X[5]
    a = np.sort(np.concatenate([[5, 2001, 2003], rng.choice(np.arange(10, 1900), 700, replace=False)])).astype(np.int64)
    b = np.sort(rng.choice(n, 1500, replace=False)).astype(np.int64)
    idx = hip.FlatIndexF16(d, metric="cosine")
    idx.add(X)
    ra, rb = idx.rowset(a), idx.rowset(b)
    per_query = [ra, rb, ra, ra, rb, ra, rb, ra]          # five queries of a (two tiles at four per tile), three of b
    rows = l2_ref.stored_rows(oracle, X, "f16", True)
    Dr, Ir = np.empty((8, 10), np.float32), np.empty((8, 10), np.int64)
    for rs, allowed in ((ra, a), (rb, b)):
        pos = [i for i, r in enumerate(per_query) if r is rs]
        Dr[pos], Ir[pos] = subset_ref.search(oracle, rows, Q[pos], 10, allowed, "ip", True)
    for strategy in ("subset", "overfetch", "auto"):
        _check(idx.search_filtered_many(Q, 10, per_query, strategy=strategy), (Dr, Ir), np.arange(8), 10, strategy)
    assert Ir[0, :3].tolist() == [5, 2001, 2003]


def test_overfetch_falls_back_for_the_group_whose_rows_rank_last(hip, oracle):
    """Group a allows the 200 rows LEAST similar to its query: k' results hold none of them and the query goes to the row
    lists; group b (half the rows, three queries) is answered by the strike alone — in the same batch."""
    M = _master()
    X, Q = M["X"], M["Q"][:4]
    idx, _, _ = _index(hip, "f16", "cosine")
    rows = l2_ref.stored_rows(oracle, X, "f16", True)
    full_I = oracle.flat_search_f16(rows, oracle.normalize_L2(Q[:1]), N)[0]
    a = np.sort(full_I[0, -200:]).astype(np.int64)
    b = np.sort(np.random.default_rng(5).choice(N, N // 2, replace=False)).astype(np.int64)
    ra, rb = idx.rowset(a), idx.rowset(b)
    before = dict(idx.filtered_stats)
    D_got, I_got = idx.search_filtered_many(Q, 10, [ra, rb, rb, rb], strategy="overfetch")
    after = idx.filtered_stats
    assert after["fallback_queries"] == before["fallback_queries"] + 1
    assert after["overfetch_batches"] == before["overfetch_batches"] + 1 and after["subset_batches"] == before["subset_batches"] + 1
    Dr, Ir = np.empty((4, 10), np.float32), np.empty((4, 10), np.int64)
    Dr[:1], Ir[:1] = subset_ref.search(oracle, rows, Q[:1], 10, a, "ip", True)
    Dr[1:], Ir[1:] = subset_ref.search(oracle, rows, Q[1:], 10, b, "ip", True)
    _check((D_got, I_got), (Dr, Ir), np.arange(4), 10, "fallback")
    assert I_got[0].tolist() == full_I[0, -200:-190].tolist()


def test_refusals_come_before_any_launch(hip):
    from rag_arc_amd.hip.binding import RarcError, RarcUnsupported

    rng = np.random.default_rng(3)
    X = rng.standard_normal((500, 64)).astype(np.float32)
    Q = rng.standard_normal((5, 64)).astype(np.float32)
    idx = hip.FlatIndexF16(64, metric="cosine")
    idx.add(X[:400])
    stale = idx.rowset([1, 2, 3])
    idx.add(X[400:])
    good = idx.rowset([4, 5, 6, 7])
    other = hip.FlatIndexF16(64, metric="cosine")
    other.add(X[:100])
    foreign = other.rowset([1, 2])
    idx.search_filtered_many(Q, 2, [good] * 5)
    before = dict(idx.filtered_stats)
    with pytest.raises(RarcError, match=r"rowsets\[3\].*changed"):
        idx.search_filtered_many(Q, 2, [good, None, good, stale, good])
    with pytest.raises(ValueError, match=r"rowsets\[1\]"):
        idx.search_filtered_many(Q, 2, [good, foreign, good, good, good])
    with pytest.raises(ValueError, match=r"rowsets\[0\]"):
        idx.search_filtered_many(Q, 2, [[4, 5], good, good, good, good])
    with pytest.raises(ValueError, match="one RowSet"):
        idx.search_filtered_many(Q, 2, [good] * 4)
    with pytest.raises(RarcUnsupported, match="8192"):
        idx.search_filtered_many(Q, 9000, [good] * 5)
    with pytest.raises(ValueError):
        idx.search_filtered_many(Q, 0, [good] * 5)
    with pytest.raises(ValueError):
        idx.search_filtered_many(Q, 2, [good] * 5, strategy="fastest")
    assert idx.filtered_stats == before
    f8 = hip.FlatIndexF16(256, metric="cosine", storage="f8")
    f8.add(rng.standard_normal((50, 256)).astype(np.float32))
    with pytest.raises(RarcUnsupported, match="'f16' or 'f32'"):
        f8.search_filtered_many(rng.standard_normal((2, 256)).astype(np.float32), 2, [None, None])
    assert f8.filtered_stats == {key: 0 for key in f8.filtered_stats}
    with pytest.raises(RarcUnsupported, match="twin"):
        idx.twin().search_filtered_many(Q, 2, [good] * 5)
    # the empty index answers padding
    empty = hip.FlatIndexF16(64, metric="l2")
    D0, I0 = empty.search_filtered_many(Q[:2], 3, [empty.rowset([]), None])
    assert (I0 == -1).all() and np.isposinf(D0).all()


# ------------------------------------------------------------------------------------------------------------------ the store
TENANTS = ["red", "green", "blue"]


def _store(**kw):
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore

    texts = [f"document {i}" for i in range(600)]
    metas = [{"tenant": TENANTS[i % 3], "year": 2018 + i % 5} for i in range(600)]
    metas[3] = {"tenant": "lonely"}                          # a tenant with ONE document: fewer matches than k
    store = HipFlatVectorStore(HashEmbeddings(64), metric="cosine", **kw)
    store.add_texts(texts, metas, ids=[f"id{i}" for i in range(600)])
    return store


def _pairs(answer):
    return [(d.id, s) for d, s in answer]


def test_store_filters_one_per_query():
    from rag_arc_amd.core.retrieval.dense import VectorStoreRetriever

    store = _store()
    queries = [f"document {7 * i + 1}" for i in range(12)]
    handle = store.row_filter({"tenant": "blue"})
    is_2020 = lambda m: m.get("year") == 2020      # noqa: E731
    filters = [{"tenant": "red"}, {"tenant": "green"}, handle, None, {"tenant": "red"}, is_2020, {"tenant": "lonely"},
               {"tenant": "nobody"}, {"tenant": "green", "year": [2019, 2021]}, None, is_2020, handle]
    want = [store.similarity_search_with_score(q, 5, filter=f) for q, f in zip(queries, filters)]
    assert [len(w) for w in want] == [5, 5, 5, 5, 5, 5, 1, 0, 5, 5, 5, 5]
    assert all(d.metadata["tenant"] == "red" for d, _ in want[0]) and all(d.metadata["year"] == 2020 for d, _ in want[5])
    before = dict(store.index.filtered_stats)
    got = store.batch_similarity_search_with_score(queries, 5, filters=filters)
    after = store.index.filtered_stats
    assert [_pairs(g) for g in got] == [_pairs(w) for w in want]
    assert after["grouped_calls"] == before["grouped_calls"] + 1
    assert after["groups"] == before["groups"] + 7           # equal dicts, the same callable, the same handle: once each
    assert [[d.id for d in g] for g in store.batch_similarity_search(queries, 5, filters=filters)] == [[d.id for d, _ in w] for w in want]
    vecs = np.asarray([store.embedding.embed_query(q) for q in queries], np.float32)
    sc, rows = store.batch_search_by_vector(vecs, 5, filters=filters)
    assert sc.shape == (12, 5) and [[f"id{r}" for r in row if r >= 0] for row in rows] == [[d.id for d, _ in w] for w in want]
    assert (rows[7] == -1).all() and np.isneginf(sc[7]).all() and sc[0].tolist() == [s for _, s in want[0]]
    retr = VectorStoreRetriever(store, search_kwargs={"k": 5})
    assert [[d.id for d in docs] for docs in retr.batch_invoke(queries, filters=filters)] == [[d.id for d, _ in w] for w in want]
    # filters of nothing but None: the unfiltered batch
    assert [_pairs(g) for g in store.batch_similarity_search_with_score(queries[:3], 5, filters=[None] * 3)] == \
        [_pairs(store.similarity_search_with_score(q, 5)) for q in queries[:3]]
    for call in (lambda: store.batch_similarity_search(queries, 5, filter={"tenant": "red"}, filters=filters),
                 lambda: store.batch_similarity_search_with_score(queries, 5, filters=filters[:3]),
                 lambda: store.batch_search_by_vector(vecs, 5, filter=handle, filters=filters),
                 lambda: store.batch_search_by_vector(vecs, 5, filters=filters + [None]),
                 lambda: retr.batch_invoke(queries, filter=handle, filters=filters),
                 lambda: retr.batch_invoke(queries, filters=filters[:2])):
        with pytest.raises(ValueError, match="filters="):
            call()


def test_store_refusals_with_filters():
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore
    from rag_arc_amd.encapsulation.database.vector_db.hip_sharded import HipShardedFlatVectorStore
    from rag_arc_amd.hip.binding import RarcUnsupported

    f8 = HipFlatVectorStore(HashEmbeddings(64), metric="cosine", storage="f8")
    f8.add_texts(["a", "b", "c"], [{"tenant": "a"}] * 3)
    with pytest.raises(RarcUnsupported, match="'f16' or 'f32'"):
        f8.batch_similarity_search(["a", "b"], 2, filters=[{"tenant": "a"}, None])
    assert [len(x) for x in f8.batch_similarity_search(["a", "b"], 2, filters=[None, None])] == [2, 2]
    sharded = HipShardedFlatVectorStore(HashEmbeddings(64), metric="cosine")
    with pytest.raises(RarcUnsupported, match="one-GPU store"):
        sharded.batch_similarity_search_with_score(["a"], 2, filters=[{"tenant": "a"}])


def test_concurrent_tenants_share_launches():
    """24 threads, each with its own tenant's filter, on one store: every answer is the sequential one, and the coalescing
    front answered them in fewer than 24 launches."""
    store = _store()
    queries = [f"document {11 * i + 2}" for i in range(24)]
    filters = [{"tenant": TENANTS[i % 3]} if i % 8 else None for i in range(24)]
    want = [_pairs(store.similarity_search_with_score(q, 6, filter=f)) for q, f in zip(queries, filters)]
    assert all(len(w) == 6 for w in want)
    launches0, served0 = store.coalesced_launches
    got, errors = [None] * 24, []
    gate = threading.Barrier(24)

    def work(i):
        try:
            gate.wait(timeout=30)
            got[i] = _pairs(store.similarity_search_with_score(queries[i], 6, filter=filters[i]))
        except BaseException as exc:  # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(24)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=60)
    assert not errors and got == want
    assert store.coalesced_launches[1] - served0 == 24 and store.coalesced_launches[0] - launches0 < 24


def test_a_stale_handle_fails_its_caller_only():
    import asyncio

    from rag_arc_amd.hip.binding import RarcError

    store = _store()
    handle = store.row_filter({"tenant": "red"})
    want = _pairs(store.similarity_search_with_score("document 9", 4, filter={"tenant": "green"}))
    assert _pairs(asyncio.run(store.asimilarity_search_with_score("document 9", 4, filter={"tenant": "green"}))) == want
    store.delete(["id1"])
    want = _pairs(store.similarity_search_with_score("document 9", 4, filter={"tenant": "green"}))
    # a batch that holds the stale handle fails as a whole, and the front answers it again one by one: the stale handle's
    # caller gets the error, the others their answers
    vec = np.asarray(store.embedding.embed_query("document 9"), np.float32)
    with pytest.raises(RarcError, match="changed"):
        store._run_query_batch([vec, vec], 4, [{"tenant": "green"}, handle])

    async def burst():
        calls = [store.asimilarity_search_with_score("document 9", 4, filter=handle if i == 2 else {"tenant": "green"}) for i in range(6)]
        return await asyncio.gather(*calls, return_exceptions=True)

    class _Batching(HashEmbeddings):                 # (the async front takes texts: it needs a provider that embeds a batch)
        def embed_queries(self, texts):
            return np.asarray(self.embed_documents(texts), np.float32)

    store.embedding = _Batching(64)
    outcomes = asyncio.run(burst())
    assert isinstance(outcomes[2], RarcError) and "changed" in str(outcomes[2])
    assert all(_pairs(o) == want for i, o in enumerate(outcomes) if i != 2)
    with pytest.raises(RarcError, match="changed"):
        store.similarity_search_with_score("document 9", 4, filter=handle)
    assert _pairs(store.similarity_search_with_score("document 9", 4, filter={"tenant": "green"})) == want
    with pytest.raises(ValueError):
        store.similarity_search("document 9", 4, filter="tenant=red")
