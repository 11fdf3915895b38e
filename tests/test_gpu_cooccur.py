"""The co-occurrence projection on the GPU (csrc/cooccur.hip, graph_db/cooccurrence.py) against the restatement
tests/cooccur_ref.py: everything is equal element for element — the rule is integer sums over sets, so there is no band.  Row
degrees straddle every degree-class boundary the library reports (rarc_cooccur_limits), the entity counts put key_bits on both
sides of the 8-bit radix passes, and the projected graph must answer personalized_pagerank and components() with the bits an
EntityGraph built from the reference's pairs gives."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: torch brings the HIP runtime both must share)

from tests import cooccur_ref as R

pytestmark = pytest.mark.gpu

FORMS = [("count", 1), ("count", 2), ("product", 1), ("product", 2)]


def _db():
    from rag_arc_amd.encapsulation.database import graph_db

    return graph_db


def _C():
    from rag_arc_amd.encapsulation.database.graph_db import cooccurrence

    return cooccurrence


def _same(got, want, what=""):
    """a Cooccurrence against the reference's Result"""
    pairs, w = (got.pairs.cpu().numpy(), got.weights.cpu().numpy().view(np.uint32)) if hasattr(got.pairs, "cpu") else (got.pairs, got.weights)
    assert pairs.dtype == np.int64 and w.dtype == np.uint32 and pairs.shape == (len(w), 2), what
    assert np.array_equal(pairs, want.pairs), (what, len(pairs), len(want.pairs))
    assert np.array_equal(w.astype(np.int64), want.weights), what
    assert (got.total_pairs, got.chunks_skipped, got.largest_weight) == (want.total_pairs, want.chunks_skipped, want.largest_weight), what


def _rows_to_mentions(rows):
    return np.array([(c, e) for c, row in enumerate(rows) for e in row], np.int64).reshape(-1, 2)


def _check_map(n_chunks, n, mentions, weights, forms=FORMS, max_mentions=64):
    mm = _db().MentionMap(n_chunks, n, mentions, weights)
    for weight, min_weight in forms:
        want = R.cooccur_mentions(n_chunks, n, mentions, weights, weight=weight, min_weight=min_weight, max_mentions=max_mentions)
        _same(mm.cooccurrence_pairs(weight=weight, min_weight=min_weight, max_mentions=max_mentions), want, (weight, min_weight, max_mentions))
    return mm


# ---- the degree classes -----------------------------------------------------------------------------------------------------------------
def test_rows_of_every_degree_class_in_one_map():
    lim = _C().limits()
    wave = lim["wave_degree"]
    assert wave == 64 and lim["max_mentions"] == 4096
    rng = np.random.default_rng(1)
    n = 300
    degrees = [0, 1, 2, 3, 8, 9, wave - 1, wave, wave + 1, 200, 2, 0, wave + 1, 5]
    rows = [np.sort(rng.permutation(n)[:d]) for d in degrees]
    mentions = _rows_to_mentions(rows)
    weights = rng.integers(1, 60, len(mentions))
    mm = _check_map(len(degrees), n, mentions, weights, max_mentions=256)               # every row contributes
    got = mm.cooccurrence_pairs(max_mentions=256)
    assert got.total_pairs == sum(d * (d - 1) // 2 for d in degrees) and got.chunks_skipped == 0
    _check_map(len(degrees), n, mentions, weights, forms=[("count", 1), ("product", 1)])  # the default guard drops 65, 200 and 65
    assert mm.cooccurrence_pairs().chunks_skipped == 3


@pytest.mark.parametrize("max_mentions", [2, 64, 100])
def test_a_row_of_exactly_max_mentions_contributes_and_one_more_does_not(max_mentions):
    rng = np.random.default_rng(max_mentions)
    n = max_mentions + 50
    rows = [np.sort(rng.permutation(n)[:d]) for d in (max_mentions, max_mentions + 1, 2, max_mentions)]
    mentions = _rows_to_mentions(rows)
    weights = rng.integers(1, 4, len(mentions))
    mm = _db().MentionMap(4, n, mentions, weights)
    for weight in ("count", "product"):
        want = R.cooccur_mentions(4, n, mentions, weights, weight=weight, max_mentions=max_mentions)
        got = mm.cooccurrence_pairs(weight=weight, max_mentions=max_mentions)
        _same(got, want, weight)
        assert got.chunks_skipped == 1 and got.total_pairs == max_mentions * (max_mentions - 1) + 1


def test_a_row_that_fills_the_staging_of_a_workgroup():
    """max_mentions at its limit: a row of exactly that many mentions fills the LDS staging, one more is dropped.  8.4 M pairs are
    too many for the Python loops of the reference: one row of distinct entities gives each of its pairs once, written down here
    with np.triu_indices."""
    top = _C().limits()["max_mentions"]
    rng = np.random.default_rng(4)
    n = top + 100
    rows = [np.sort(rng.permutation(n)[:top]), np.sort(rng.permutation(n)[:top + 1])]
    mentions = _rows_to_mentions(rows)
    weights = rng.integers(1, 1 << 12, len(mentions))
    got = _db().MentionMap(2, n, mentions, weights).cooccurrence_pairs(weight="product", max_mentions=top)
    i, j = np.triu_indices(top, k=1)                                                       # row-major: ascending (a, b), as the row ascends
    assert got.total_pairs == len(i) == top * (top - 1) // 2 and got.chunks_skipped == 1
    assert np.array_equal(got.pairs, np.stack([rows[0][i], rows[0][j]], axis=1))
    w0 = weights[:top].astype(np.int64)
    assert np.array_equal(got.weights.astype(np.int64), w0[i] * w0[j]) and got.largest_weight == int((w0[i] * w0[j]).max())


def test_pairs_repeated_across_many_chunks_and_a_min_weight_above_the_largest():
    rng = np.random.default_rng(3)
    n_chunks, n = 400, 12                                                                  # few entities: every pair many times
    mentions = np.stack([rng.integers(0, n_chunks, 2400), rng.integers(0, n, 2400)], axis=1)
    weights = rng.integers(1, 30, len(mentions))
    mm = _check_map(n_chunks, n, mentions, weights)
    for weight in ("count", "product"):
        top = mm.cooccurrence_pairs(weight=weight).largest_weight
        assert top > 20
        want = R.cooccur_mentions(n_chunks, n, mentions, weights, weight=weight, min_weight=top)
        _same(mm.cooccurrence_pairs(weight=weight, min_weight=top), want)
        assert 1 <= len(want.pairs) < n * (n - 1) // 2
        got = mm.cooccurrence_pairs(weight=weight, min_weight=top + 1)                     # an empty answer, not an error
        assert got.pairs.shape == (0, 2) and got.weights.shape == (0,) and got.largest_weight == top and got.total_pairs == want.total_pairs
        dev = mm.cooccurrence_pairs(weight=weight, min_weight=top + 1, as_device=True)
        assert dev.pairs.is_cuda and tuple(dev.pairs.shape) == (0, 2) and tuple(dev.weights.shape) == (0,)
    with pytest.raises(ValueError, match="no two entities share a chunk"):
        mm.cooccurrence(min_weight=10 ** 9)


@pytest.mark.parametrize("n", [2, 16, 17, 257, 70000])
def test_entity_counts_on_both_sides_of_the_radix_passes(n):
    """key_bits = 2 ceil(log2 n): 2, 8, 10, 18 and 34; entities 0 and n - 1 are mentioned together"""
    rng = np.random.default_rng(n)
    n_chunks = 300
    d = np.minimum(rng.integers(0, 7, n_chunks), n)
    rows = [np.sort(rng.permutation(min(n, 5000))[:k] * (n // min(n, 5000))) for k in d]
    rows[0] = np.array([0, n - 1])
    rows[1] = np.array([0, n - 1]) if n == 2 else np.array([0, n // 2, n - 1])
    mentions = _rows_to_mentions(rows)
    weights = rng.integers(1, 1 << 12, len(mentions))
    mm = _check_map(n_chunks, n, mentions, weights)
    got = mm.cooccurrence_pairs()
    assert got.pairs[0, 0] == 0 and [0, n - 1] in got.pairs.tolist()


# ---- a CSR adopted from the device --------------------------------------------------------------------------------------------------
def _adopt(n_chunks, n, row_ptr, ent, w):
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dt)).cuda()                           # noqa: E731
    return _db().MentionMap.from_device_csr(n_chunks, n, t(row_ptr, np.int64), t(ent, np.int32), t(np.asarray(w, np.uint32).view(np.int32), np.int32))


def test_an_adopted_csr_with_entries_outside_the_rule_and_a_repeated_entity():
    from rag_arc_amd.hip import binding as B

    n = 50
    # row 0: e >= n, w = 0, w = 2^12, e < 0 between good entries; row 1: a repeated entity; row 2: only bad entries; row 3: good
    row_ptr = [0, 8, 12, 14, 17]
    ent = [3, n, 5, 7, 9, -1, 11, n + 9, 20, 20, 21, 20, -5, n, 0, 30, n - 1]
    w = [2, 1, 0, 4096, 4095, 1, 3, 1, 2, 3, 4, 5, 1, 1, 7, 8, 9]
    mm = _adopt(4, n, row_ptr, ent, w)
    for weight in ("count", "product"):
        want = R.cooccur(row_ptr, ent, w, n, weight=weight)
        assert want.entries_skipped == 7 and want.total_pairs == 3 + 6 + 0 + 3
        _same(mm.cooccurrence_pairs(weight=weight), want, weight)
        assert not any(a == b for a, b in want.pairs.tolist())
    assert R.cooccur(row_ptr, ent, w, n, weight="product").weights[[2, 3, 4, 5]].tolist() == [2 * 4095, 2 * 3, 4095 * 3, 8 + 12 + 20]
    lib = B.load_library()                                                                 # the counts of the C entry itself
    ws = torch.empty(int(lib.rarc_cooccur_workspace_bytes(4, len(ent))), dtype=torch.uint8, device="cuda")
    out4 = torch.empty(4, dtype=torch.int64, device="cuda")
    B.check(lib.rarc_cooccur_count(mm._row_ptr.data_ptr(), mm._ent.data_ptr(), mm._w.data_ptr(), 4, len(ent), n, 3, ws.data_ptr(), ws.numel(),
                                   out4.data_ptr(), None), "rarc_cooccur_count")
    torch.cuda.synchronize()
    want = R.cooccur(row_ptr, ent, w, n, max_mentions=3)
    assert out4.tolist() == [want.total_pairs, want.contributing, want.chunks_skipped, want.entries_skipped] == [6, 2, 1, 7]


def test_a_map_adopted_with_from_device_csr_equals_the_host_built_one():
    rng = np.random.default_rng(8)
    n_chunks, n = 500, 333
    mentions = np.stack([rng.integers(0, n_chunks, 3000), rng.integers(0, n, 3000)], axis=1)
    weights = rng.integers(1, 9, len(mentions))
    host = _db().MentionMap(n_chunks, n, mentions, weights)
    adopted = _db().MentionMap.from_device_csr(n_chunks, n, host._row_ptr.clone(), host._ent.clone(), host._w.clone())
    for weight, min_weight in FORMS:
        a, b = (m.cooccurrence_pairs(weight=weight, min_weight=min_weight) for m in (host, adopted))
        _same(a, R.cooccur_mentions(n_chunks, n, mentions, weights, weight=weight, min_weight=min_weight))
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- a larger random map --------------------------------------------------------------------------------------------------------------
N_CHUNKS, N = 20011, 5003


@pytest.fixture(scope="module")
def heavy():
    """about 20,000 chunks over 5,000 entities: most chunks mention 1 .. 8 entities, a heavy tail up to 300, popular entities often"""
    rng = np.random.default_rng(17)
    d = np.minimum((rng.pareto(1.6, N_CHUNKS) * 2).astype(np.int64) + 1, 300)
    d[rng.integers(0, N_CHUNKS, 200)] = 0
    ent = np.minimum((rng.pareto(1.1, int(d.sum())) * 40).astype(np.int64), N - 1)       # a few entities are in very many chunks
    mentions = np.stack([np.repeat(np.arange(N_CHUNKS), d), ent], axis=1)
    weights = rng.integers(1, 6, len(mentions))
    refs = {(w, k): R.cooccur_mentions(N_CHUNKS, N, mentions, weights, weight=w, max_mentions=k) for w, k in (("count", 64), ("product", 128))}
    return mentions, weights, refs


def test_a_heavy_tailed_random_map(heavy):
    mentions, weights, refs = heavy
    mm = _db().MentionMap(N_CHUNKS, N, mentions, weights)
    assert refs[("count", 64)].chunks_skipped > 0                                          # the tail reaches past the default guard
    for (weight, k), want in refs.items():
        assert want.total_pairs > 100000 and want.largest_weight > 50
        _same(mm.cooccurrence_pairs(weight=weight, max_mentions=k), want, (weight, k))


def test_shuffled_mentions_two_runs_and_the_device_form_give_identical_bits(heavy):
    mentions, weights, refs = heavy
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(mentions))
    a = _db().MentionMap(N_CHUNKS, N, mentions, weights)
    b = _db().MentionMap(N_CHUNKS, N, mentions[perm], weights[perm])
    first = a.cooccurrence_pairs(weight="product", max_mentions=128)
    for other in (b.cooccurrence_pairs(weight="product", max_mentions=128), a.cooccurrence_pairs(weight="product", max_mentions=128)):
        assert all(np.array_equal(x, y) for x, y in zip(first, other))
    dev = a.cooccurrence_pairs(weight="product", max_mentions=128, as_device=True)
    assert dev.pairs.is_cuda and dev.weights.is_cuda and dev.pairs.dtype == torch.int64 and dev.weights.dtype == torch.int32
    assert np.array_equal(dev.pairs.cpu().numpy(), first.pairs) and np.array_equal(dev.weights.cpu().numpy().view(np.uint32), first.weights)
    assert dev[2:] == first[2:]
    _same(dev, refs[("product", 128)])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_the_projected_graph_answers_as_one_built_from_the_reference_pairs(heavy):
    mentions, weights, refs = heavy
    db = _db()
    want = refs[("count", 64)]
    mm = db.MentionMap(N_CHUNKS, N, mentions, weights)
    g, ref = mm.cooccurrence(), db.EntityGraph(N, want.pairs, weights=want.weights)
    assert (g.n, g.m) == (ref.n, ref.m) == (N, len(want.pairs))
    assert np.array_equal(g._pairs.cpu().numpy(), ref._pairs.cpu().numpy()) and np.array_equal(g._pair_weights.cpu().numpy(), ref._pair_weights.cpu().numpy())
    seeds = [[0], [1, 17, N - 1], [100, 101, 102]]
    assert np.array_equal(g.personalized_pagerank(seeds).view(np.uint64), ref.personalized_pagerank(seeds).view(np.uint64))
    for x, y in zip(g.rank_chunks(mm, seeds, top_k=20), ref.rank_chunks(mm, seeds, top_k=20)):
        assert np.array_equal(x, y)
    for x, y in zip(g.components(), ref.components()):
        assert np.array_equal(x, y)
    one = db.cooccurrence_graph(N_CHUNKS, N, mentions, weights)                            # the one-call form
    assert np.array_equal(one._pairs.cpu().numpy(), g._pairs.cpu().numpy())


def test_the_projection_of_a_merged_map_equals_the_reference_on_the_merged_mentions():
    from tests import merge_ref as M

    db = _db()
    rng = np.random.default_rng(23)
    n_chunks, n = 700, 900
    mentions = np.stack([rng.integers(0, n_chunks, 5000), rng.integers(0, n, 5000)], axis=1)
    weights = rng.integers(1, 9, len(mentions))
    labels = M.planted_labels(n, 100, 4)
    plan = M.plan(labels)
    merged = db.merge_entities(labels, mentions=db.MentionMap(n_chunks, n, mentions, weights))
    mm, mw, _ = M.merge_mentions(plan["new_id"], n_chunks, mentions, weights)
    assert merged.plan.n_merged == plan["n_merged"] < n
    for weight in ("count", "product"):
        _same(merged.mentions.cooccurrence_pairs(weight=weight), R.cooccur_mentions(n_chunks, plan["n_merged"], mm, mw, weight=weight), weight)


def test_a_retriever_without_pairs_returns_the_documents_of_one_given_the_reference_pairs():
    from rag_arc_amd.core.retrieval import HipGraphRetriever
    from tests import passage_ref as P
    from tests.helpers import HashEmbeddings

    n_ent, n_chunks = 40, 30
    entities = [f"entity {i}" for i in range(n_ent)]
    chunks = [f"chunk {i} of the corpus" for i in range(n_chunks)]
    ids = [f"c{i}" for i in range(n_chunks)]
    mentions, mw = P.random_mentions(n_ent, n_chunks, seed=22, max_degree=4, max_weight=9)
    emb = HashEmbeddings(64)
    x = np.asarray(emb.embed_documents(entities), np.float32)
    queries = ["entity 3", "entity 17", "who founded entity 5", "an unrelated question"]
    for kw, ref_kw in (({}, {}), ({"cooccurrence_weight": "product", "min_weight": 2, "max_mentions": 3},
                                 {"weight": "product", "min_weight": 2, "max_mentions": 3})):
        want = R.cooccur_mentions(n_chunks, n_ent, mentions, mw, **ref_kw)
        assert len(want.pairs) > 5
        a = HipGraphRetriever.from_arrays(emb, x, None, mentions, chunks, mention_weights=mw, ids=ids, k=5, **kw)
        b = HipGraphRetriever.from_arrays(emb, x, want.pairs, mentions, chunks, pair_weights=want.weights, mention_weights=mw, ids=ids, k=5)
        assert a.graph.m == b.graph.m == len(want.pairs)
        for da, db_ in zip(a.batch_invoke(queries, k=6), b.batch_invoke(queries, k=6)):
            assert [(d.id, d.content, d.score) for d in da] == [(d.id, d.content, d.score) for d in db_] and len(da) > 0
