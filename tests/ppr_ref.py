"""Personalized PageRank as csrc/ppr.hip defines it, in Python integers — and the same rule in float64 without
the floors, to bound what the floors cost.

    ONE = 2^40, a = round(damping * 65536), W(u) = u's weighted degree
    t_q(v) = sum over q's seed slots (v, w) of (w << 40) // Wq,  Wq = the sum of q's slot weights;  p_0 = t_q
    c(u) = p(u) // W(u);  flow(v) = sum over neighbours u of w_uv * c(u)  (W(v) = 0: flow(v) = p(v))
    p'(v) = ((65536 - a) * t_q(v) + a * flow(v)) >> 16
    after each step delta = max_v |p' - p|; delta <= floor(tolerance * ONE) ends the query

Every query is computed on its own: a batch is its rows one by one, by construction."""
ONE = 1 << 40
MAX_SEED_WEIGHT = 1 << 20


def damping_q16(damping):
    a = int(round(float(damping) * 65536))
    assert 0 <= a < 65536
    return a


def tolerance_units(tolerance):
    return int(float(tolerance) * ONE)


def adjacency(n, edges, weights=None):
    """rows of (neighbour, weight) and the weighted degrees; edges are undirected pairs, each once"""
    adj = [[] for _ in range(n)]
    W = [0] * n
    for e, (a, b) in enumerate(edges):
        w = 1 if weights is None else int(weights[e])
        assert 0 <= a < n and 0 <= b < n and a != b and w >= 1
        adj[a].append((b, w))
        adj[b].append((a, w))
        W[a] += w
        W[b] += w
    return adj, W


def teleport(n, seeds, seed_weights=None):
    """seeds: vertices (-1 = unused slot); weights: integers 0 .. 2^20, unit by default"""
    ws = [1] * len(seeds) if seed_weights is None else [int(w) for w in seed_weights]
    assert all(0 <= w <= MAX_SEED_WEIGHT for w in ws)
    wq = sum(w for v, w in zip(seeds, ws) if v >= 0)
    t = [0] * n
    if wq:
        for v, w in zip(seeds, ws):
            if v >= 0:
                t[v] += (w << 40) // wq
    return t


def step(adj, W, t, p, a):
    c = [p[u] // W[u] if W[u] else 0 for u in range(len(p))]
    out = []
    for v in range(len(p)):
        flow = sum(w * c[u] for u, w in adj[v]) if W[v] else p[v]
        out.append(((65536 - a) * t[v] + a * flow) >> 16)
    return out


def ppr_one(n, edges, seeds, seed_weights=None, weights=None, damping=0.85, max_iterations=20, tolerance=0.0, graph=None):
    """-> (p as a list of n integers, iterations run)"""
    adj, W = graph if graph is not None else adjacency(n, edges, weights)
    a, tol = damping_q16(damping), tolerance_units(tolerance)
    t = teleport(n, seeds, seed_weights)
    p = list(t)
    it = 0
    while it < max_iterations:
        nxt = step(adj, W, t, p, a)
        delta = max(abs(x - y) for x, y in zip(nxt, p))
        p = nxt
        it += 1
        if delta <= tol:
            break
    return p, it


def ppr(n, edges, seed_lists, seed_weight_lists=None, **kw):
    """a batch: the rows one by one -> (list of p, list of iterations run)"""
    graph = adjacency(n, edges, kw.pop("weights", None))
    out = [ppr_one(n, edges, s, None if seed_weight_lists is None else seed_weight_lists[i], graph=graph, **kw)
           for i, s in enumerate(seed_lists)]
    return [p for p, _ in out], [it for _, it in out]


def ppr_batch(n, edges, seed_lists, seed_weight_lists=None, weights=None, damping=0.85, max_iterations=20, tolerance=0.0):
    """`ppr` for shapes the Python integers are too slow for: the same rule in numpy uint64 over the whole batch
    -> (uint64 array [B][n], list of iterations run).  The Python-integer functions above stay the definition: this one is
    trusted only because tests/test_ppr_batch_ref_host.py finds it equal to them, element for element.
    Every intermediate is asserted below 2^63 (csrc/ppr.hip's header proves 2^57), so no uint64 wraps unseen."""
    import numpy as np

    def u64(x):
        x = np.asarray(x)
        assert x.size == 0 or int(x.max()) < 1 << 63
        return x.astype(np.uint64, copy=False)

    B = len(seed_lists)
    a, tol = damping_q16(damping), tolerance_units(tolerance)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    w = np.ones(len(e), np.int64) if weights is None else np.asarray(weights, dtype=np.int64)
    assert w.shape == (len(e),) and (len(e) == 0 or (e.min() >= 0 and e.max() < n and (e[:, 0] != e[:, 1]).all() and w.min() >= 1))
    src, dst = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])       # the doubled edge list: flow goes src -> dst
    w2 = u64(np.concatenate([w, w]))
    W = np.zeros(n, np.int64)
    np.add.at(W, src, np.concatenate([w, w]))
    W = u64(W)
    linked = W > 0
    t = np.zeros((B, n), np.uint64)
    for q, seeds in enumerate(seed_lists):
        ws = None if seed_weight_lists is None else seed_weight_lists[q]
        t[q] = u64(np.array(teleport(n, seeds, ws), dtype=np.uint64))                       # Python integers <= 2^40: the same floors
    p = t.copy()
    its = [0] * B
    live = np.ones(B, bool)
    safe_W = np.where(linked, W, np.uint64(1))
    for _ in range(max_iterations):
        rows = np.flatnonzero(live)
        if rows.size == 0:
            break
        pl = p[rows]
        c = np.where(linked[None, :], pl // safe_W[None, :], np.uint64(0))
        terms = u64(c[:, src] * w2[None, :])                                                # w_uv * c(u) <= p(u) <= 2^40
        flow = np.zeros_like(pl)
        np.add.at(flow, (np.arange(rows.size)[:, None], dst[None, :]), terms)
        flow = u64(np.where(linked[None, :], flow, pl))
        nxt = u64(np.uint64(65536 - a) * t[rows] + np.uint64(a) * flow) >> np.uint64(16)
        delta = np.where(nxt > pl, nxt - pl, pl - nxt).max(axis=1)
        p[rows] = nxt
        for i, q in enumerate(rows):
            its[q] += 1
            if int(delta[i]) <= tol:
                live[q] = False
    return p, its


def scores(p):
    """p / ONE as floats: exact, p <= 2^40 < 2^53"""
    return [x / ONE for x in p]


def topk(p, k):
    """(ids, scores, count): the vertices of positive score by (score descending, vertex ascending), cut at k, (-1, -inf) behind"""
    order = sorted((v for v in range(len(p)) if p[v] > 0), key=lambda v: (-p[v], v))[:k]
    pad = k - len(order)
    return order + [-1] * pad, [p[v] / ONE for v in order] + [float("-inf")] * pad, len(order)


def quantise_weights(ws):
    """float weights -> integers: scaled so the largest is 1, then round(w * 2^20) (half to even, as numpy and the GPU path do)"""
    import numpy as np

    w = np.asarray(ws, dtype=np.float64)
    mx = w.max() if w.size else 0.0
    if not mx > 0:
        return [0] * len(w)
    return [int(x) for x in np.rint(w / mx * float(MAX_SEED_WEIGHT))]


# ---- the same rule in float64, without floors ----------------------------------------------------------------------------------------
def ppr_float(n, edges, seeds, seed_weights=None, weights=None, damping=0.85, max_iterations=20):
    """p as floats summing to 1 (or 0): the exact-arithmetic rule the integers approximate; damping = a / 65536 exactly"""
    adj, W = adjacency(n, edges, weights)
    d = damping_q16(damping) / 65536.0
    ws = [1] * len(seeds) if seed_weights is None else list(seed_weights)
    wq = float(sum(w for v, w in zip(seeds, ws) if v >= 0))
    t = [0.0] * n
    if wq:
        for v, w in zip(seeds, ws):
            if v >= 0:
                t[v] += w / wq
    p = list(t)
    for _ in range(max_iterations):
        c = [p[u] / W[u] if W[u] else 0.0 for u in range(n)]
        p = [(1.0 - d) * t[v] + d * (sum(w * c[u] for u, w in adj[v]) if W[v] else p[v]) for v in range(n)]
    return p


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
def path_graph(n):
    return [(i, i + 1) for i in range(n - 1)]


def star_graph(leaves):
    """hub 0 with `leaves` neighbours"""
    return leaves + 1, [(0, i) for i in range(1, leaves + 1)]


def complete_bipartite(a, b):
    """K(a, b): left vertices 0 .. a - 1, right vertices a .. a + b - 1 -> (n, edges)"""
    return a + b, [(i, a + j) for i in range(a) for j in range(b)]


def with_hub(n, edges, d, weights=None, max_weight=1):
    """one more vertex, n, joined to the vertices 0 .. d - 1 with weights 1 .. max_weight in turn -> (n + 1, edges, weights)"""
    assert 1 <= d <= n
    ws = [1] * len(edges) if weights is None else list(weights)
    return n + 1, list(edges) + [(v, n) for v in range(d)], ws + [1 + v % max_weight for v in range(d)]


def degrees(n, edges):
    """the number of neighbours of every vertex (edges are undirected pairs, each once)"""
    deg = [0] * n
    for a, b in edges:
        deg[a] += 1
        deg[b] += 1
    return deg


def random_graph(n, m, seed, max_weight=1):
    import random

    rng = random.Random(seed)
    edges = set()
    while len(edges) < m:
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b:
            edges.add((min(a, b), max(a, b)))
    edges = sorted(edges)
    return edges, [rng.randint(1, max_weight) for _ in edges]


def two_components_and_isolated():
    """a 6-cycle, a 4-path with a chord, and vertices 10, 11, 12 without an edge"""
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (0, 5), (6, 7), (7, 8), (8, 9), (6, 8)]
    return 13, edges
