"""Entity merging on the GPU (csrc/merge.hip, graph_db/merge.py) against the restatement tests/merge_ref.py: everything is equal
element for element — the rule is integer sums, maxima and scans, so there is no band.  The sort is taken at the edges of its
tile (T = what rarc_sort_reduce_limits reports), of a wave (63, 64, 65) and of a digit (key_bits 1, 8, 9, 33, 62), and on keys
that differ in one digit only, which an unstable pass would scramble.  The planted graph has about 2,000 vertices; merged objects
must answer personalized_pagerank, rank_chunks, neighbourhood and subgraph with the bits the host constructors' objects give."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: torch brings the HIP runtime both must share)

from tests import merge_ref as R

pytestmark = pytest.mark.gpu


def _M():
    from rag_arc_amd.encapsulation.database.graph_db import merge

    return merge


def _db():
    from rag_arc_amd.encapsulation.database import graph_db

    return graph_db


def _same_sort(keys, values, key_bits, **kw):
    got_k, got_s, got_max = _M().sort_reduce(keys, values, key_bits=key_bits, **kw)
    want_k, want_s, want_max = R.sort_reduce(keys, values)
    assert got_k.dtype == np.uint64 and got_s.dtype == np.uint64
    assert np.array_equal(got_k, want_k), (len(keys), key_bits, np.argwhere(got_k[:len(want_k)] != want_k[:len(got_k)])[:5])
    assert np.array_equal(got_s, want_s) and got_max == want_max, (len(keys), key_bits)


# ---- rarc_sort_reduce -----------------------------------------------------------------------------------------------------------------
def _counts():
    t = _M().limits()["tile"]
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 3 * t + 1]


@pytest.mark.parametrize("key_bits", [1, 8, 9, 33, 62])
def test_sort_reduce_at_every_count_and_key_width(key_bits):
    rng = np.random.default_rng(key_bits)
    assert _M().limits()["tile"] == 2048
    for count in _counts():
        # few distinct keys (long runs that cross chunks and tiles) and, where the width allows, mostly distinct ones
        for distinct in (7, 1 << 40):
            keys = rng.integers(0, min(distinct, 1 << key_bits), count, dtype=np.uint64)
            if key_bits > 8:
                keys[rng.integers(0, count, 3)] = (1 << key_bits) - 1          # the top bit of the top digit is used
            _same_sort(keys, rng.integers(0, 1 << 32, count, dtype=np.uint64), key_bits)
            _same_sort(keys, None, key_bits)


def test_sort_reduce_on_equal_sorted_and_reversed_keys():
    t = _M().limits()["tile"]
    n = 3 * t + 1
    vals = np.arange(n, dtype=np.uint64) % 1000
    _same_sort(np.full(n, 123456789, np.uint64), vals, 33)
    got = _M().sort_reduce(np.full(n, 5, np.uint64), None, key_bits=8)
    assert got[0].tolist() == [5] and got[1].tolist() == [n] and got[2] == n
    asc = np.arange(n, dtype=np.uint64) * 3
    _same_sort(asc, vals, 16)
    _same_sort(asc[::-1].copy(), vals, 16)


def test_a_pass_is_stable_keys_that_differ_in_one_digit_only():
    """The order of equal digits must survive every later pass: with keys that differ only in the lowest digit the higher passes
    see equal digits everywhere, with keys that differ only in the highest used digit the lower ones do.  The values make the
    sums tell which key an element was filed under."""
    rng = np.random.default_rng(3)
    n = 5000
    low = rng.integers(0, 256, n, dtype=np.uint64)
    vals = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    _same_sort((np.uint64(0x1234_5678_9A) << np.uint64(8)) | low, vals, 48)
    _same_sort((low << np.uint64(40)) | np.uint64(0x77_6655_4433), vals, 48)
    _same_sort((low << np.uint64(54)) | np.uint64(0x3F_FFFF_FFFF_FFFF), vals, 62)


def test_a_sum_that_passes_2_to_the_32_is_carried_whole_and_device_tensors_are_taken_where_they_are():
    import torch

    n = 300
    keys = np.arange(n, dtype=np.uint64) % 3
    vals = np.full(n, (1 << 32) - 1, np.uint64)
    k, s, mx = _M().sort_reduce(keys, vals, key_bits=2)
    assert k.tolist() == [0, 1, 2] and s.tolist() == [100 * ((1 << 32) - 1)] * 3 and mx == 100 * ((1 << 32) - 1) > 1 << 32
    dk = torch.from_numpy(keys.view(np.int64)).cuda()
    dv = torch.from_numpy(vals.astype(np.uint32).view(np.int32)).cuda()
    k2, s2, mx2 = _M().sort_reduce(dk, dv, key_bits=2, as_device=True)
    assert k2.is_cuda and k2.cpu().tolist() == [0, 1, 2] and s2.cpu().tolist() == s.tolist() and mx2 == mx
    assert dk.cpu().numpy().view(np.uint64).tolist() == keys.tolist()                  # the inputs are only read


# ---- the plan -----------------------------------------------------------------------------------------------------------------------
def _same_plan(labels, richness=None, **kw):
    host = [None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else x) for x in (labels, richness)]
    got, want = _M().merge_plan(labels, richness, **kw), R.plan(*host)
    assert (got.n, got.n_merged) == (want["n"], want["n_merged"])
    for k in ("primary", "new_id", "kept", "removed"):
        g = getattr(got, k)
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == np.int64 and np.array_equal(g, want[k]), k
    return got


@pytest.mark.parametrize("n", [1, 2, 257, 5000])
def test_plans(n):
    import torch

    rng = np.random.default_rng(n)
    p = _same_plan(np.arange(n))                                                       # all singletons
    assert p.n_merged == n and p.removed.size == 0
    p = _same_plan(np.full(n, n - 1))                                                  # one class, its label its largest member
    assert p.n_merged == 1 and p.kept.tolist() == [0]
    p = _same_plan(np.zeros(n, np.int64), np.full(n, 7))                               # every richness ties: the smallest index
    assert p.kept.tolist() == [0]
    rich = rng.integers(0, 3, n)
    rich[rng.integers(0, n)] = (1 << 32) - 1
    labels = rng.integers(0, n, n)                                                     # labels that are no member's index
    _same_plan(labels, rich)
    _same_plan(torch.from_numpy(labels).cuda(), torch.from_numpy(rich).cuda(), as_device=True)
    _same_plan(R.planted_labels(n, n // 8, n), rich)


# ---- pairs, mentions and relations on a planted graph ---------------------------------------------------------------------------------
N, N_CHUNKS = 2003, 701


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(11)
    labels = R.planted_labels(N, 120, 4)
    rich = rng.integers(0, 4, N)
    e = rng.integers(0, N, (6000, 2))
    e = e[e[:, 0] != e[:, 1]]
    groups = [np.flatnonzero(labels == c) for c in np.unique(labels) if (labels == c).sum() > 1]
    inside = np.array([[g[0], g[1]] for g in groups])                                  # pairs that fall inside an entity
    pairs = np.unique(np.sort(np.concatenate([e, inside]), axis=1), axis=0)
    weights = rng.integers(1, 50, len(pairs))
    ment = np.stack([rng.integers(0, N_CHUNKS, 9000), rng.integers(0, N, 9000)], axis=1)
    # chunk 5 mentions the members of 70 different entities: its merged row crosses the split degree of 64
    ment = np.concatenate([ment, np.stack([np.full(150, 5), rng.permutation(N)[:150]], axis=1)])
    mw = rng.integers(1, 9, len(ment))
    rel = np.concatenate([e[rng.permutation(len(e))][:5000], inside[:, ::-1], np.stack([np.arange(0, N, 7)] * 2, axis=1), [[-1, 3], [4, N]]])
    rel = rel[rng.permutation(len(rel))]
    return {"labels": labels, "rich": rich, "pairs": pairs, "weights": weights, "ment": ment, "mw": mw, "rel": rel,
            "rw": rng.standard_normal(len(rel)).astype(np.float32), "plan": R.plan(labels, rich)}


def _host_objects(p, shuffle=None):
    db = _db()
    rng = np.random.default_rng(0 if shuffle is None else shuffle)
    po, mo = (np.arange(len(p["pairs"])), np.arange(len(p["ment"]))) if shuffle is None else (rng.permutation(len(p["pairs"])),
                                                                                              rng.permutation(len(p["ment"])))
    pairs = p["pairs"][po]
    if shuffle is not None:
        flip = rng.random(len(pairs)) < 0.5
        pairs = np.where(flip[:, None], pairs[:, ::-1], pairs)
    return (db.EntityGraph(N, pairs, weights=p["weights"][po]), db.MentionMap(N_CHUNKS, N, p["ment"][mo], p["mw"][mo]),
            db.RelationList(N, p["rel"], weights=p["rw"]))


def _reference_objects(p):
    """what the host route builds: tests/merge_ref.py's output through the existing host constructors"""
    db, new_id, n_c = _db(), p["plan"]["new_id"], p["plan"]["n_merged"]
    rp, rw, de, dw = R.merge_pairs(new_id, p["pairs"], p["weights"])
    mm, mw, _ = R.merge_mentions(new_id, N_CHUNKS, p["ment"], p["mw"])
    table, rows, internal, out = R.merge_relations(new_id, p["rel"])
    objs = (db.EntityGraph(n_c, rp, weights=rw), db.MentionMap(N_CHUNKS, n_c, mm, mw), db.RelationList(n_c, table, weights=p["rw"][rows]))
    return objs, {"pairs": rp, "weights": rw, "rows": rows, "table": table,
                  "dropped": {"edges": de, "edge_weight": dw, "relations_internal": internal, "relations_out_of_range": out}}


def _bits(m):
    """every buffer of a MergedEntities, on the host"""
    g, mm, rl = m.graph, m.mentions, m.relations
    return [g._pairs.cpu().numpy(), g._pair_weights.cpu().numpy(), mm._row_ptr.cpu().numpy(), mm._ent.cpu().numpy(), mm._w.cpu().numpy(),
            mm._split.cpu().numpy(), rl._pairs.cpu().numpy(), rl._weights.cpu().numpy(), np.asarray(m.relation_rows)]


@pytest.fixture(scope="module")
def merged(planted):
    g, mm, rl = _host_objects(planted)
    before = [x.clone() for x in (g._pairs, g._pair_weights, mm._row_ptr, mm._ent, mm._w, rl._pairs)]
    out = _M().merge_entities(planted["labels"], graph=g, mentions=mm, relations=rl, richness=planted["rich"])
    after = (g._pairs, g._pair_weights, mm._row_ptr, mm._ent, mm._w, rl._pairs)
    assert all(bool((a == b).all()) for a, b in zip(before, after))                    # the inputs are not modified
    return out


def test_the_merged_buffers_equal_the_reference(planted, merged):
    from rag_arc_amd.encapsulation.database.graph_db.passages import mention_csr

    _, want = _reference_objects(planted)
    new_id, n_c = planted["plan"]["new_id"], planted["plan"]["n_merged"]
    assert merged.plan.n_merged == n_c < N and np.array_equal(merged.plan.new_id, new_id)
    assert merged.dropped == want["dropped"] and want["dropped"]["edges"] >= 100 and want["dropped"]["relations_out_of_range"] == 2
    assert merged.graph.n == n_c and merged.graph.m == len(want["pairs"])
    assert np.array_equal(merged.graph._pairs.cpu().numpy(), want["pairs"])
    assert np.array_equal(merged.graph._pair_weights.cpu().numpy().view(np.uint32), want["weights"])
    mm, mw, _ = R.merge_mentions(new_id, N_CHUNKS, planted["ment"], planted["mw"])
    row_ptr, ent, w, split = mention_csr(N_CHUNKS, n_c, mm, mw)
    got = merged.mentions
    assert (got.n_chunks, got.n_entities, got.nnz, got.n_split) == (N_CHUNKS, n_c, len(ent), len(split))
    assert np.array_equal(got._row_ptr.cpu().numpy(), row_ptr) and np.array_equal(got._ent.cpu().numpy(), ent)
    assert np.array_equal(got._w.cpu().numpy().view(np.uint32), w)
    assert 5 in split and np.array_equal(got._split.cpu().numpy(), split)              # the merged row of chunk 5 crosses the split degree
    assert row_ptr[6] - row_ptr[5] > got.split_degree
    assert merged.relations.r == len(want["rows"]) and np.array_equal(merged.relation_rows, want["rows"])
    assert np.array_equal(merged.relations._pairs.cpu().numpy(), want["table"])
    assert np.array_equal(merged.relations._weights.cpu().numpy(), planted["rw"][want["rows"]])
    self_rows = planted["rel"][want["rows"]]
    assert (self_rows[:, 0] == self_rows[:, 1]).sum() == len(np.arange(0, N, 7))       # a == b stays, on a removed entity too


def test_shuffled_input_and_device_input_give_the_same_bits(planted, merged):
    import torch

    want = _bits(merged)
    g, mm, rl = _host_objects(planted, shuffle=9)
    for a, b in zip(_bits(_M().merge_entities(planted["labels"], graph=g, mentions=mm, relations=rl, richness=planted["rich"])), want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    db = _db()
    pw = torch.from_numpy(planted["weights"]).cuda()
    g = db.EntityGraph(N, torch.from_numpy(planted["pairs"]).cuda(), weights=pw)
    rl = db.RelationList(N, torch.from_numpy(planted["rel"]).cuda(), weights=torch.from_numpy(planted["rw"]).cuda())
    plan = _M().merge_plan(torch.from_numpy(planted["labels"]).cuda(), torch.from_numpy(planted["rich"]).cuda(), as_device=True)
    out = _M().merge_entities(plan, graph=g, mentions=mm, relations=rl, as_device=True)
    assert out.relation_rows.is_cuda and out.plan.kept.is_cuda
    for a, b in zip(_bits(out._replace(relation_rows=out.relation_rows.cpu().numpy())), want):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    again = _bits(_M().merge_entities(plan, graph=g, mentions=mm, relations=rl))       # and from run to run
    assert all(np.array_equal(a, b) for a, b in zip(again, want))


def test_merged_objects_answer_as_the_host_built_ones(planted, merged):
    (g, mm, rl), _ = _reference_objects(planted)
    n_c = merged.plan.n_merged
    seeds = [[0], [5, 17, n_c - 1], [100, 101, 102, 103], []]
    for a, b in ((merged.graph, g),):
        assert np.array_equal(a.personalized_pagerank(seeds[:3]).view(np.uint64), b.personalized_pagerank(seeds[:3]).view(np.uint64))
        for x, y in zip(a.personalized_pagerank(seeds[:3], top_k=50), b.personalized_pagerank(seeds[:3], top_k=50)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.rank_chunks(merged.mentions, seeds[:3]).view(np.uint64), b.rank_chunks(mm, seeds[:3]).view(np.uint64))
        for x, y in zip(a.rank_chunks(merged.mentions, seeds[:3], top_k=20), b.rank_chunks(mm, seeds[:3], top_k=20)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.neighbourhood(seeds, hops=2), b.neighbourhood(seeds, hops=2))
        for rel_a, rel_b in ((None, None), (merged.relations, rl)):
            sa = a.subgraph(seeds, hops=2, max_vertices=500, max_edges=700, relations=rel_a)
            sb = b.subgraph(seeds, hops=2, max_vertices=500, max_edges=700, relations=rel_b)
            assert sa._fields == sb._fields and sa.edge_counts.sum() > 0
            for x, y in zip(sa, sb):
                assert x.dtype == y.dtype and np.array_equal(x, y)


def test_a_merge_that_leaves_no_edge_returns_no_graph_and_a_table_of_internal_rows_no_relations():
    db = _db()
    g = db.EntityGraph(4, [(0, 1), (2, 3)], weights=[3, 4])
    rl = db.RelationList(4, [(1, 0), (3, 2)])
    out = _M().merge_entities([0, 0, 3, 3], graph=g, relations=rl)
    assert out.graph is None and out.relations is None and out.relation_rows.tolist() == []
    assert out.dropped == {"edges": 2, "edge_weight": 7, "relations_internal": 2, "relations_out_of_range": 0} and out.plan.n_merged == 2
    out = _M().merge_entities([0, 0, 0, 0], graph=g)                                    # one vertex remains
    assert out.graph is None and out.plan.n_merged == 1
    out = _M().merge_entities([0, 1, 1, 3], graph=g)                                    # (0, 1), (2, 3) -> (0, 1), (1, 2)
    assert out.graph._pairs.cpu().tolist() == [[0, 1], [1, 2]] and out.dropped["edges"] == 0


def test_a_mention_sum_of_2_to_the_12_is_refused_and_one_below_is_accepted():
    from rag_arc_amd.hip import binding as B

    db = _db()
    mm = db.MentionMap(3, 4, [(1, 0), (1, 2), (1, 3), (0, 1)], [4000, 95, 1, 7])
    out = _M().merge_entities([0, 1, 0, 3], mentions=mm)                                # 4000 + 95 = 2^12 - 1
    assert out.mentions._w.cpu().tolist() == [7, 4095, 1] and out.mentions._ent.cpu().tolist() == [1, 0, 2]
    assert out.mentions._row_ptr.cpu().tolist() == [0, 1, 3, 3] and out.mentions.n_split == 0
    with pytest.raises(B.RarcUnsupported, match="4096"):
        _M().merge_entities([0, 1, 0, 0], mentions=mm)                                  # 4000 + 95 + 1 = 2^12


# ---- steps 1 - 4 in one call ----------------------------------------------------------------------------------------------------------
def test_deduplicate_entities_equals_entity_clusters_followed_by_the_reference_merge():
    from tests.test_gpu_louvain import GROUP_SIZES

    db = _db()
    rng = np.random.default_rng(5)
    rows, group = [], []
    for gi, size in enumerate(GROUP_SIZES):                                             # the planted groups of test_gpu_louvain.py
        c = rng.standard_normal(64)
        c /= np.linalg.norm(c)
        rows.append(c + 0.01 * rng.standard_normal((size, 64)))
        group += [gi] * size
    perm = rng.permutation(len(group))
    x = np.concatenate(rows)[perm].astype(np.float32)
    n = len(x)
    rich = rng.integers(0, 5, n)
    e = rng.integers(0, n, (3000, 2))
    pairs = np.unique(np.sort(e[e[:, 0] != e[:, 1]], axis=1), axis=0)
    ment = np.stack([rng.integers(0, 50, 800), rng.integers(0, n, 800)], axis=1)
    g, mm, rl = db.EntityGraph(n, pairs), db.MentionMap(50, n, ment), db.RelationList(n, e)
    got = db.deduplicate_entities(x, richness=rich, graph=g, mentions=mm, relations=rl)
    labels = db.entity_clusters(x, as_labels=True)
    want = R.plan(labels, rich)
    assert want["n_merged"] == len(GROUP_SIZES) == got.plan.n_merged
    for k in ("primary", "new_id", "kept", "removed"):
        assert np.array_equal(getattr(got.plan, k), want[k]), k
    rp, rw, de, dw = R.merge_pairs(want["new_id"], pairs)
    assert np.array_equal(got.graph._pairs.cpu().numpy(), rp) and np.array_equal(got.graph._pair_weights.cpu().numpy(), rw)
    wm, ww, _ = R.merge_mentions(want["new_id"], 50, ment)
    ref = db.MentionMap(50, want["n_merged"], wm, ww)
    assert all(np.array_equal(getattr(got.mentions, k).cpu().numpy(), getattr(ref, k).cpu().numpy()) for k in ("_row_ptr", "_ent", "_w"))
    table, rws, internal, _ = R.merge_relations(want["new_id"], e)
    assert np.array_equal(got.relations._pairs.cpu().numpy(), table) and np.array_equal(got.relation_rows, rws)
    assert got.dropped == {"edges": de, "edge_weight": dw, "relations_internal": internal, "relations_out_of_range": 0}
