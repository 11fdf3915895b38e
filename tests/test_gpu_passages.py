"""EntityGraph.rank_chunks / retrieve_chunks on the GPU (csrc/ppr.hip, the passage projection) against the integer restatement
tests/passage_ref.py: the [B][n_chunks] scores (S / 2^28, exact) and the top-k ids, scores and counts are equal bit for bit —
the rule is integer arithmetic, so there is no band.  The shapes are the smallest that reach each form of the kernel: both
forms, a partial wave and a second one, the 16-byte form and the odd batch that falls off it, a chunk one below, at and above
the degree at which it is split across a workgroup, chunks without mentions, twins, the largest key, the kernel's own guard.
Of ppr_chunks_kernel<BP, QPL, SPLIT> the first cases reach BP = 1, 4, 32 and 64 (2 and 8 only in passing: two device-side
queries, five for the twins, seven in retrieve_chunks), split at B = 1, 3, 64, 65 only;
test_the_random_map_in_the_chunk_parallel_forms_between adds BP = 2, 8 and 16, test_a_split_chunk_in_every_form the split form
at every BP and with two queries per lane, and the two strided cases a grid-stride walk of each launch (their references are
the numpy forms of ppr_ref and passage_ref, proved equal to the Python integers by tests/test_ppr_batch_ref_host.py).  The
step's own forms are in tests/test_gpu_ppr.py and tests/test_gpu_ppr_forms.py; DESIGN §4.13e lists instantiation x launch -> case."""
import random

import numpy as np
import pytest

from tests import passage_ref as P
from tests import ppr_ref as R

pytestmark = pytest.mark.gpu


def _graph(n, edges, weights=None):
    from rag_arc_amd.encapsulation.database.graph_db import EntityGraph

    return EntityGraph(n, edges, weights=weights)


def _map(n_chunks, n, mentions, weights=None):
    from rag_arc_amd.encapsulation.database.graph_db import MentionMap

    return MentionMap(n_chunks, n, mentions, weights=weights)


def _seed_sets(n, count, rng):
    """`count` queries of 1 .. 6 seeds with integer weights; duplicates happen"""
    seeds = [[rng.randrange(n) for _ in range(rng.randint(1, 6))] for _ in range(count)]
    return seeds, [[rng.randint(1, 50) for _ in s] for s in seeds]


def _ref_states(n, edges, seeds, seed_w, weights=None, **kw):
    sw = None if seed_w is None else [R.quantise_weights(w) for w in seed_w]
    return R.ppr(n, edges, seeds, sw, weights=weights, **kw)[0]


def _check(n, edges, n_chunks, mentions, mweights, seeds, seed_w, weights=None, ks=(), g=None, mm=None, states=None, **kw):
    """scores bit for bit, then every k of ks: ids, scores, counts -> the reference S per query"""
    states = states if states is not None else _ref_states(n, edges, seeds, seed_w, weights, **kw)
    want = [P.chunk_state(p, n_chunks, mentions, mweights) for p in states]
    g = g if g is not None else _graph(n, edges, weights)
    mm = mm if mm is not None else _map(n_chunks, n, mentions, mweights)
    got = g.rank_chunks(mm, seeds, seed_w, **kw)
    assert got.dtype == np.float64 and got.shape == (len(seeds), n_chunks)
    assert np.array_equal(got, np.asarray([P.scores(S) for S in want]))
    for k in ks:
        ids, sc, cnt = g.rank_chunks(mm, seeds, seed_w, top_k=k, **kw)
        assert ids.dtype == np.int64 and sc.dtype == np.float64 and cnt.dtype == np.int32
        for q, S in enumerate(want):
            wi, wsc, wc = P.topk(S, k)
            assert cnt[q] == wc and ids[q].tolist() == wi and sc[q].tolist() == wsc, (k, q)
    return want


def test_one_chunk_one_mention_on_one_edge_and_an_empty_chunk_between_two():
    for damping in (0.0, 0.85):
        _check(2, [(0, 1)], 1, [(0, 1)], None, [[0], [1], [0, 1]], None, ks=(1, 2), damping=damping)
        want = _check(5, R.path_graph(5), 3, [(0, 1), (2, 3), (2, 4), (0, 0)], [3, 1, 4095, 17], [[0], [2], [4, 0]],
                      [[1.0], [0.3], [0.25, 1.0]], ks=(1, 3, 6), damping=damping)
        assert all(S[1] == 0 for S in want)                       # never ranked: every count is at most 2
        assert all(P.topk(S, 3)[2] <= 2 for S in want)


@pytest.fixture(scope="module")
def g200():
    n = 200
    edges, weights = R.random_graph(n, 600, seed=11, max_weight=5)
    mentions, mweights = P.random_mentions(n, 150, seed=12)
    return {"n": n, "edges": edges, "weights": weights, "n_chunks": 150, "mentions": mentions, "mweights": mweights,
            "g": _graph(n, edges, weights), "mm": _map(150, n, mentions, mweights)}


def _args(f):
    return (f["n"], f["edges"], f["n_chunks"], f["mentions"], f["mweights"])


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("batch", [1, 3, 64, 65])
def test_a_chunk_around_the_split_degree(g200, delta, batch):
    """chunk 1 has one mention fewer than a single wave walks, exactly as many, and one more (the split form); chunk 0 and 2
    are ordinary, chunk 3 has none"""
    from rag_arc_amd.encapsulation.database.graph_db.passages import limits

    n, d = g200["n"], limits()["split_degree"] + delta
    big, bw = P.chunk_of_degree(n, d, seed=20 + delta, chunk=1)
    mentions, mweights = [(0, 5), (2, 9), (2, 5)] + big, [7, 4095, 1] + bw
    mm = _map(4, n, mentions, mweights)
    assert mm.n_split == (1 if delta > 0 else 0)
    seeds, w = _seed_sets(n, batch, random.Random(100 + delta))
    _check(n, g200["edges"], 4, mentions, mweights, seeds, w, weights=g200["weights"], ks=(4,), g=g200["g"], mm=mm, max_iterations=5)


@pytest.mark.parametrize("batch", [1, 3, 32, 33, 64, 65, 130])
def test_a_random_weighted_graph_in_every_form(g200, batch):
    """B = 1, 3, 32: chunk-parallel; 33, 64: query-parallel within one wave; 65: a second, partial wave (odd: one query per lane);
    130: two queries and one 16-byte load per lane"""
    seeds, w = _seed_sets(g200["n"], batch, random.Random(batch))
    _check(*_args(g200), seeds, w, weights=g200["weights"], ks=(1, 10, 150, 157) if batch <= 3 else (10,), g=g200["g"], mm=g200["mm"])


def _chunk_form(batch):
    """(BP, QPL, chunks of queries) of the ppr_chunks_kernel instantiation rarc_ppr_chunks picks: the step's own rule"""
    from rag_arc_amd.encapsulation.database.graph_db.pagerank import limits

    if batch > limits()["vertex_parallel_max_batch"]:
        qpl = 2 if batch > 64 and batch % 2 == 0 else 1
        return 64, qpl, -(-batch // (64 * qpl))
    bp = 1
    while bp < batch:
        bp *= 2
    return bp, 1, 1


def _batch_states(f, seeds, seed_w, **kw):
    """the PPR states of a batch from ppr_ref's numpy form (proved equal to the Python integers on the host) -> uint64 [B][n]"""
    return R.ppr_batch(f["n"], f["edges"], seeds, [R.quantise_weights(w) for w in seed_w], weights=f["weights"], **kw)[0]


@pytest.mark.parametrize("batch", [2, 5, 8, 9, 16, 17])
def test_the_random_map_in_the_chunk_parallel_forms_between(g200, batch):
    """BP = 2, 8 (B = 5 and 8), 16 (9 and 16) and 32 at its smallest batch: the instantiations the cases above pass over"""
    assert _chunk_form(batch)[:2] == {2: (2, 1), 5: (8, 1), 8: (8, 1), 9: (16, 1), 16: (16, 1), 17: (32, 1)}[batch]
    seeds, w = _seed_sets(g200["n"], batch, random.Random(500 + batch))
    _check(*_args(g200), seeds, w, weights=g200["weights"], ks=(10,), g=g200["g"], mm=g200["mm"])


@pytest.mark.parametrize("batch", [2, 8, 16, 32, 66, 130, 256])
def test_a_split_chunk_in_every_form(g200, batch):
    """chunk 1 has one mention more than a single wave walks: the split form at every BP the cases above leave out, and with two
    queries per lane (66, 130, 256); chunk 0 and 2 are ordinary, chunk 3 has none"""
    from rag_arc_amd.encapsulation.database.graph_db.passages import limits

    want_form = {2: (2, 1, 1), 8: (8, 1, 1), 16: (16, 1, 1), 32: (32, 1, 1), 66: (64, 2, 1), 130: (64, 2, 2), 256: (64, 2, 2)}
    assert _chunk_form(batch) == want_form[batch]
    n, d = g200["n"], limits()["split_degree"] + 1
    big, bw = P.chunk_of_degree(n, d, seed=600 + batch, chunk=1)
    mentions, mweights = [(0, 5), (2, 9), (2, 5)] + big, [7, 4095, 1] + bw
    mm = _map(4, n, mentions, mweights)
    assert mm.n_split == 1 and mm.nnz == d + 3
    seeds, w = _seed_sets(n, batch, random.Random(600 + batch))
    states = _batch_states(g200, seeds, w, max_iterations=5).tolist()
    want = _check(n, g200["edges"], 4, mentions, mweights, seeds, w, weights=g200["weights"], ks=(4,), g=g200["g"], mm=mm, states=states,
                  max_iterations=5)
    assert all(S[1] > 0 and S[3] == 0 for S in want)


def _check_batch(f, n_chunks, mentions, mweights, mm, batch, seed, rows, k=5):
    """a map too large for passage_ref's Python integers: the scores in full against its numpy form, the top-k of `rows`"""
    seeds, w = _seed_sets(f["n"], batch, random.Random(seed))
    want = P.chunk_states_batch(_batch_states(f, seeds, w, max_iterations=5), n_chunks, mentions, mweights)
    got = f["g"].rank_chunks(mm, seeds, w, max_iterations=5)
    assert got.dtype == np.float64 and got.shape == (batch, n_chunks)
    assert np.array_equal(got, want.astype(np.float64) / float(P.SCORE_ONE))      # S < 2^40: both steps exact
    ids, sc, cnt = f["g"].rank_chunks(mm, seeds, w, max_iterations=5, top_k=k)
    for q in rows:
        wi, wsc, wc = P.topk(want[q].tolist(), k)
        assert cnt[q] == wc and ids[q].tolist() == wi and sc[q].tolist() == wsc, q
    return want


def test_a_strided_walk_over_17000_chunks(g200):
    """17000 chunks of one to three mentions at B = 65: 2 chunks of queries, 34000 items for the plain launch's 8192 workgroups of
    4 waves; the chunks from 16384 on are some wave's second visit"""
    n, n_chunks, batch = g200["n"], 17000, 65
    assert _chunk_form(batch) == (64, 1, 2) and n_chunks * 2 > 8192 * 4
    rng = random.Random(700)
    mentions = [(c, e) for c in range(n_chunks) for e in rng.sample(range(n), 1 + c % 3)]
    mweights = [rng.randint(1, P.MAX_WEIGHT - 1) for _ in mentions]
    mm = _map(n_chunks, n, mentions, mweights)
    assert mm.n_split == 0
    want = _check_batch(g200, n_chunks, mentions, mweights, mm, batch, seed=701, rows=(0, 31, 64))
    assert want[:, 8192 * 4 // 2:].any(axis=1).all()


def test_a_strided_split_walk_over_1100_chunks(g200):
    """1100 chunks of 65 mentions at B = 65: every chunk is split, 2200 items for the split launch's 2048 workgroups"""
    from rag_arc_amd.encapsulation.database.graph_db.passages import limits

    n, n_chunks, batch, d = g200["n"], 1100, 65, limits()["split_degree"] + 1
    assert _chunk_form(batch) == (64, 1, 2) and n_chunks * 2 > 2048 and d == 65
    mentions, mweights = [], []
    for c in range(n_chunks):
        ms, ws = P.chunk_of_degree(n, d, seed=800 + c, chunk=c)
        mentions += ms
        mweights += ws
    mm = _map(n_chunks, n, mentions, mweights)
    assert mm.n_split == n_chunks
    want = _check_batch(g200, n_chunks, mentions, mweights, mm, batch, seed=801, rows=(0, 31, 64))
    assert want[:, 2048 // 2:].any(axis=1).all()


def test_the_largest_key_damping_0_one_seed_weight_4095(g200):
    n = g200["n"]
    mentions, mweights = [(0, 9), (1, 9), (2, 10), (1, 9)], [4095, 4000, 4095, 95]
    want = _check(n, g200["edges"], 3, mentions, mweights, [[9]], None, weights=g200["weights"], ks=(1, 3), g=g200["g"], damping=0.0)
    assert want[0] == [4095 << 28, 4095 << 28, 0]               # all the mass on the seed; the twins are ordered by id (checked above)


def test_twin_chunks_are_ordered_by_id(g200):
    mentions, mweights = P.random_mentions(g200["n"], 40, seed=3, max_degree=6)
    mentions, mweights = [(c + 1, e) for c, e in mentions], list(mweights)               # chunk 0 is free
    src = next(c for c, _ in mentions if c > 20)
    mentions, mweights = P.with_twins(mentions, mweights, src=src, dst=0)
    seeds, w = _seed_sets(g200["n"], 5, random.Random(6))
    want = _check(g200["n"], g200["edges"], 41, mentions, mweights, seeds, w, weights=g200["weights"], ks=(41,), g=g200["g"])
    for S in want:
        assert S[0] == S[src]
        if S[0]:
            ids = P.topk(S, 41)[0]
            assert ids.index(0) < ids.index(src)


def test_k_of_1_of_n_chunks_and_beyond_and_a_query_without_weight(g200):
    seeds = [[3], [17, 150, 17], [5, 6]]
    w = [[1.0], [0.5, 1.0, 0.25], [0.0, 0.0]]
    want = _check(*_args(g200), seeds, w, weights=g200["weights"], ks=(1, 150, 158), g=g200["g"], mm=g200["mm"])
    assert want[2] == [0] * 150 and P.topk(want[2], 4) == ([-1] * 4, [float("-inf")] * 4, 0)
    assert 0 < P.topk(want[0], 158)[2] < 150                      # padding past the count, chunks without mentions left out


def test_permuted_mentions_and_split_weights_give_the_same_bits(g200):
    seeds, w = _seed_sets(g200["n"], 40, random.Random(1))
    want = g200["g"].rank_chunks(g200["mm"], seeds, w)
    order = list(range(len(g200["mentions"])))
    random.Random(2).shuffle(order)
    permuted = _map(150, g200["n"], [g200["mentions"][i] for i in order], [g200["mweights"][i] for i in order])
    assert np.array_equal(g200["g"].rank_chunks(permuted, seeds, w), want)
    m2, w2 = P.split_weights(g200["mentions"], g200["mweights"], seed=4)
    split = _map(150, g200["n"], m2, w2)
    assert split.nnz == g200["mm"].nnz < len(m2)
    assert np.array_equal(g200["g"].rank_chunks(split, seeds, w), want)
    a, b = g200["g"].rank_chunks(split, seeds, w, top_k=7), g200["g"].rank_chunks(g200["mm"], seeds, w, top_k=7)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_queries_freeze_on_their_own_under_a_tolerance(g200):
    n, edges, weights = g200["n"], g200["edges"], g200["weights"]
    seeds = [[3], [17, 150, 17], [5, 6, 7, 8], [199]] + _seed_sets(n, 36, random.Random(4))[0]
    states, its = R.ppr(n, edges, seeds, weights=weights, tolerance=3e-3, max_iterations=30)
    assert len(set(its)) > 2 and max(its) < 30
    _check(*_args(g200), seeds, None, weights=weights, ks=(5,), g=g200["g"], mm=g200["mm"], states=states, tolerance=3e-3, max_iterations=30)
    got = g200["g"].rank_chunks(g200["mm"], seeds, tolerance=3e-3, max_iterations=30)
    for q in (0, 1, 39):
        assert np.array_equal(g200["g"].rank_chunks(g200["mm"], [seeds[q]], tolerance=3e-3, max_iterations=30)[0], got[q])


def test_a_batch_of_300_is_its_rows(g200):
    g, mm = g200["g"], g200["mm"]
    seeds, w = _seed_sets(g200["n"], 300, random.Random(5))
    got = g.rank_chunks(mm, seeds, w, max_iterations=6)
    ids, sc, cnt = g.rank_chunks(mm, seeds, w, max_iterations=6, top_k=5)
    assert got.shape == (300, 150) and ids.shape == (300, 5)
    for q in list(range(0, 300, 23)) + [255, 256, 299]:
        assert np.array_equal(g.rank_chunks(mm, [seeds[q]], [w[q]], max_iterations=6)[0], got[q])
        oi, osc, oc = g.rank_chunks(mm, [seeds[q]], [w[q]], max_iterations=6, top_k=5)
        assert oi[0].tolist() == ids[q].tolist() and osc[0].tolist() == sc[q].tolist() and oc[0] == cnt[q]
    states = _ref_states(g200["n"], g200["edges"], seeds[250:260], w[250:260], g200["weights"], max_iterations=6)
    want = [P.scores(P.chunk_state(p, 150, g200["mentions"], g200["mweights"])) for p in states]
    assert np.array_equal(got[250:260], np.asarray(want))


def test_the_vertex_ranking_is_not_disturbed(g200):
    """the projection only reads the PPR workspace and keeps its keys in a workspace of its own"""
    g, mm = g200["g"], g200["mm"]
    seeds, w = _seed_sets(g200["n"], 70, random.Random(8))
    before = g.personalized_pagerank(seeds, w, top_k=5)
    scores_before = g.personalized_pagerank(seeds, w)
    g.rank_chunks(mm, seeds, w, top_k=9)
    g.rank_chunks(mm, seeds[:3], w[:3])
    after = g.personalized_pagerank(seeds, w, top_k=5)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert np.array_equal(g.personalized_pagerank(seeds, w), scores_before)
    want = _ref_states(g200["n"], g200["edges"], seeds[:4], w[:4], g200["weights"])
    assert [after[0][q].tolist() for q in range(4)] == [R.topk(p, 5)[0] for p in want]


def test_device_outputs(g200):
    import torch

    seeds = torch.tensor([[4, 9, -1], [150, -1, -1]], dtype=torch.int64).cuda()
    out = g200["g"].rank_chunks(g200["mm"], seeds, as_device=True)
    assert out.is_cuda and out.dtype == torch.float64
    states, _ = R.ppr(g200["n"], g200["edges"], [[4, 9, -1], [150, -1, -1]], weights=g200["weights"])
    want = [P.chunk_state(p, 150, g200["mentions"], g200["mweights"]) for p in states]
    assert np.array_equal(out.cpu().numpy(), np.asarray([P.scores(S) for S in want]))
    ids, sc, cnt = g200["g"].rank_chunks(g200["mm"], seeds, top_k=3, as_device=True)
    assert ids.is_cuda and sc.is_cuda and cnt.is_cuda and ids[0].tolist() == P.topk(want[0], 3)[0]


def test_retrieve_chunks_seeds_from_the_index_then_ranks_chunks(g200):
    """row i of a 200 x 64 fp16 index is vertex i: the seeds are index.search's own answer, the state is ppr_ref's and the
    ranking passage_ref's"""
    from rag_arc_amd.hip.engine import FlatIndexF16

    n = g200["n"]
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, 64)).astype(np.float32)
    x[:, 0] += 6.0                                            # every row leans towards e0: a query along -e0 scores them all below 0
    e0 = np.zeros((1, 64), np.float32)
    e0[0, 0] = 1.0
    queries = np.concatenate([x[:3] + 0.1 * rng.standard_normal((3, 64)).astype(np.float32), -e0, e0,
                              rng.standard_normal((2, 64)).astype(np.float32)])
    index = FlatIndexF16(64, metric="cosine", device=0)
    index.add(x)
    D, I = index.search(queries, 5)
    ids, sc, cnt = g200["g"].retrieve_chunks(index, queries, g200["mm"], seeds_per_query=5, top_k=10)
    graph = R.adjacency(n, g200["edges"], g200["weights"])
    for q in range(len(queries)):
        w = R.quantise_weights(np.clip(D[q].astype(np.float64), 0.0, None))
        p, _ = R.ppr_one(n, g200["edges"], I[q].tolist(), w, graph=graph)
        wi, wsc, wc = P.topk(P.chunk_state(p, 150, g200["mentions"], g200["mweights"]), 10)
        assert ids[q].tolist() == wi and sc[q].tolist() == wsc and cnt[q] == wc
    assert (D[3] < 0).all() and cnt[3] == 0 and ids[3].tolist() == [-1] * 10      # scores clipped at 0: a query without weight
    other = FlatIndexF16(64, metric="cosine", device=0)
    other.add(x[:150])
    with pytest.raises(ValueError, match="150 rows"):
        g200["g"].retrieve_chunks(other, queries, g200["mm"])


@pytest.mark.parametrize("batch", [3, 65, 130])
def test_the_kernels_own_guard(g200, batch):
    """Through the raw binding: a CSR in which one entry names entity n (exactly one past the last vertex) and one has weight 0
    gives the same S as the CSR without them.  Even unguarded, row n of p would lie inside the PPR workspace (its next state
    follows p), so this cannot fault; negative and large ids are covered by the Python-side refusals."""
    import torch

    from rag_arc_amd.encapsulation.database.graph_db.passages import mention_csr
    from rag_arc_amd.hip import binding as B

    g, n, m = g200["g"], g200["n"], len(g200["edges"])
    seeds, w = _seed_sets(n, batch, random.Random(40 + batch))
    clean = [(0, 5), (0, 9), (1, 9), (2, 7), (2, 8), (2, 150)]
    cw = [3, 4095, 17, 1, 2, 5]
    want = g.rank_chunks(_map(3, n, clean, cw), seeds, w)
    # the same CSR with two entries more in chunk 1: (entity n, weight 9) and (entity 11, weight 0); and one in chunk 2 with
    # weight 2^12, one past the largest
    row_ptr, ent, wt, _ = mention_csr(3, n, clean, cw)
    ent2 = np.concatenate([ent[:3], [n, 11], ent[3:], [12]]).astype(np.int32)
    wt2 = np.concatenate([wt[:3], [9, 0], wt[3:], [1 << 12]]).astype(np.uint32)
    rp2 = np.asarray([0, 2, 5, 9], np.int64)
    assert rp2[-1] == len(ent2) == len(wt2) and row_ptr.tolist() == [0, 2, 3, 6]
    lib = B.load_library()
    with torch.cuda.device(g.device):
        sd, wd = g._seed_tensors(seeds, w)
        cur = g._iterate(sd, wd, int(round(0.85 * 65536)), 0, 20)
        d_rp, d_ent = torch.from_numpy(rp2).cuda(), torch.from_numpy(ent2).cuda()
        d_w = torch.from_numpy(wt2.view(np.int32)).cuda()
        cws = torch.empty(int(lib.rarc_ppr_chunks_workspace_bytes(3, batch)), dtype=torch.uint8, device=g.device)
        out = torch.empty((batch, 3), dtype=torch.float64, device=g.device)
        stream = torch.cuda.current_stream().cuda_stream
        B.check(lib.rarc_ppr_chunks(n, m, batch, cur, g._ws.data_ptr(), g._ws.numel(), d_rp.data_ptr(), d_ent.data_ptr(), d_w.data_ptr(), 3,
                                    len(ent2), None, 0, cws.data_ptr(), cws.numel(), stream), "rarc_ppr_chunks")
        B.check(lib.rarc_ppr_chunks_scores(3, batch, cws.data_ptr(), cws.numel(), out.data_ptr(), stream), "rarc_ppr_chunks_scores")
        got = out.cpu().numpy()
    assert np.array_equal(got, want) and want[:, 1].any()


def test_refusals_come_before_any_launch(g200):
    from unittest import mock

    from rag_arc_amd.encapsulation.database.graph_db import MentionMap
    from rag_arc_amd.hip import binding as B

    g, mm, n = g200["g"], g200["mm"], g200["n"]
    refusing = mock.Mock(side_effect=AssertionError("a launch"))
    with mock.patch.object(g, "_run", refusing):
        for nc, ne, mentions, kw in ((3, n, [(0, n)], {}), (3, n, [(0, -1)], {}), (3, n, [(3, 0)], {}), (3, n, [(-1, 0)], {}), (3, n, [], {})):
            with pytest.raises(ValueError):
                MentionMap(nc, ne, mentions, **kw)
        with pytest.raises(B.RarcUnsupported, match="4096.*2\\^12"):
            MentionMap(3, n, [(0, 1), (0, 1), (1, 1)], weights=[4095, 1, 1])
        with pytest.raises(ValueError, match=f"{n - 1} entities"):
            g.rank_chunks(_map(3, n - 1, [(0, 1)]), [[1]])
        with pytest.raises(ValueError, match="MentionMap"):
            g.rank_chunks([(0, 1)], [[1]])
        for seeds, kw in (([list(range(65))], {}), ([], {}), ([[n]], {}), ([[1]], {"seed_weights": [[-1.0]]}), ([[1]], {"damping": 1.0}),
                          ([[1]], {"top_k": 0}), ([[1]], {"top_k": 8193}), ([[1]], {"tolerance": -1.0}), ([[1]], {"max_iterations": -1})):
            with pytest.raises(ValueError):
                g.rank_chunks(mm, seeds, **kw)
        with mock.patch.object(mm, "n_chunks", 1 << 24):      # the argument check suffices: nothing that large is allocated
            with pytest.raises(B.RarcUnsupported, match="2\\^24"):
                g.rank_chunks(mm, [[1]], top_k=5)
    assert not refusing.called
    assert B.load_library().rarc_ppr_chunks_workspace_bytes(150, 0) == 0
