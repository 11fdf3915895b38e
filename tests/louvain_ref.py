"""The Louvain rule of DESIGN §4.13c restated in plain Python integers: the normative definition csrc/louvain.hip must agree with
label for label (tests/test_gpu_louvain.py) and step for step (tests/test_gpu_louvain_steps.py), and the host checks of the rule
itself (tests/test_louvain_ref_host.py).

One input, one answer: n vertices, m unique undirected edges (i, j) with i < j, each of weight 1 -> labels[v] = the smallest
original vertex of v's community.  Nothing depends on the order of the edge list.  Python integers do not overflow; the kernels
do the same arithmetic in int64, which holds every product for m < 2^30.

A level's graph: vertices 0 .. n_l - 1, integer edge weights, self-loops from level 1 on.  k_v = weighted degree (a loop of
weight w adds 2 w), M2 = sum k_v (the same at every level).  Quality as an integer: Qn = sum_C (M2 in_C - tot_C^2), tot_C = sum
of k_v over C, in_C = twice the weight inside C (loops included); modularity = Qn / M2^2.

A sweep t is synchronous (everything is read from the state at its start).  v is a mover iff bit (16 + t mod 16) of
(v * 2654435761) mod 2^32 is 0.  A mover v in A looks at every community C != A among its neighbours:
G(C) = M2 (w_C - w_A) - k_v (tot_C - (tot_A - k_v)), w_X = weight of v's edges into X without its own loop.  Target = largest G,
ties to the smallest label, and only if G > 0; two singletons merge only towards the smaller label.  A sweep in which no mover
has a target is idle (two in a row end the level); one whose movers have targets but are all held back by the singleton rule
changes nothing and is neither idle nor tested; otherwise the sweep is kept iff Qn rose, and a sweep that is not kept ends the level.
At most max_iterations sweeps per level, idle ones included.  After a level: stop if no two vertices share a community; else
renumber the communities in ascending label order, sum the weights per community pair (inside weight -> self-loop), repeat, at
most max_levels levels."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple

HASH = 2654435761


def is_mover(v: int, t: int) -> bool:
    return (((v * HASH) & 0xFFFFFFFF) >> (16 + t % 16)) & 1 == 0


def normalise(n: int, edges: Iterable[Tuple[int, int]]) -> List[Tuple[int, int]]:
    """Swap to i < j, drop duplicates; ValueError for a loop or an index outside [0, n)."""
    out = set()
    for a, b in edges:
        a, b = int(a), int(b)
        if a == b or not (0 <= a < n and 0 <= b < n):
            raise ValueError(f"edge ({a}, {b}) on {n} vertices")
        out.add((a, b) if a < b else (b, a))
    return sorted(out)


def quality(adj: List[Dict[int, int]], loops: List[int], k: List[int], m2: int, comm: List[int]) -> int:
    """Qn of a labelling of one level's graph."""
    tot: Dict[int, int] = {}
    inside = 0
    for v, c in enumerate(comm):
        tot[c] = tot.get(c, 0) + k[v]
        inside += 2 * loops[v]
        for u, w in adj[v].items():          # every non-loop edge is seen from both ends: twice its weight
            if comm[u] == c:
                inside += w
    return m2 * inside - sum(t * t for t in tot.values())


def sweep(adj, loops, k, m2, comm: List[int], t: int) -> Tuple[List[int], int]:
    """One synchronous sweep: (new labels, how many vertices moved, how many movers had a target)."""
    n = len(comm)
    tot: Dict[int, int] = {}
    size: Dict[int, int] = {}
    for v in range(n):
        tot[comm[v]] = tot.get(comm[v], 0) + k[v]
        size[comm[v]] = size.get(comm[v], 0) + 1
    new = list(comm)
    moved = targets = 0
    for v in range(n):
        if not adj[v] or not is_mover(v, t):
            continue
        a = comm[v]
        w_to: Dict[int, int] = {}
        for u, w in adj[v].items():
            w_to[comm[u]] = w_to.get(comm[u], 0) + w
        w_a = w_to.get(a, 0)
        best_g, best_c = 0, -1
        for c, w_c in w_to.items():
            if c == a:
                continue
            g = m2 * (w_c - w_a) - k[v] * (tot[c] - (tot[a] - k[v]))
            if g > best_g or (g == best_g and best_c >= 0 and c < best_c):
                best_g, best_c = g, c
        if best_c < 0:
            continue
        targets += 1
        if size[a] == 1 and size[best_c] == 1 and not best_c < a:
            continue
        new[v] = best_c
        moved += 1
    return new, moved, targets


def run_level(adj, loops, k, m2, max_iterations: int, trace: Optional[list] = None) -> List[int]:
    n = len(adj)
    comm = list(range(n))
    best = quality(adj, loops, k, m2, comm)
    if trace is not None:
        trace.append(("level", n, best))
    idle = 0
    for t in range(max_iterations):
        new, moved, targets = sweep(adj, loops, k, m2, comm, t)
        if moved == 0:
            idle = idle + 1 if targets == 0 else 0
            if idle == 2:
                break
            continue
        idle = 0
        q = quality(adj, loops, k, m2, new)
        if trace is not None:
            trace.append(("sweep", t, moved, q))
        if q <= best:
            break
        comm, best = new, q
    return comm


def aggregate(adj, loops, comm: List[int]):
    """(new adjacency, new loops, old community label -> new vertex)."""
    ids = {c: i for i, c in enumerate(sorted(set(comm)))}
    n_c = len(ids)
    nadj: List[Dict[int, int]] = [dict() for _ in range(n_c)]
    nloops = [0] * n_c
    for v, c in enumerate(comm):
        a = ids[c]
        nloops[a] += loops[v]
        for u, w in adj[v].items():
            if u < v:
                continue
            b = ids[comm[u]]
            if a == b:
                nloops[a] += w
            else:
                nadj[a][b] = nadj[a].get(b, 0) + w
                nadj[b][a] = nadj[b].get(a, 0) + w
    return nadj, nloops, ids


def louvain(n: int, edges, max_iterations: int = 10, max_levels: int = 10, trace: Optional[list] = None) -> List[int]:
    """labels[v] = the smallest original vertex of v's community.  edges: unique (i, j), i < j (see `normalise`)."""
    if max_iterations < 1 or max_levels < 1:
        raise ValueError("max_iterations and max_levels must be at least 1")
    adj: List[Dict[int, int]] = [dict() for _ in range(n)]
    for a, b in edges:
        a, b = int(a), int(b)
        assert 0 <= a < b < n and b not in adj[a], (a, b)
        adj[a][b] = 1
        adj[b][a] = 1
    loops = [0] * n
    labels = list(range(n))                    # original vertex -> vertex of the current level
    for _ in range(max_levels):
        k = [sum(adj[v].values()) + 2 * loops[v] for v in range(len(adj))]
        m2 = sum(k)
        if m2 == 0:
            break
        comm = run_level(adj, loops, k, m2, max_iterations, trace)
        n_l = len(adj)
        adj, loops, ids = aggregate(adj, loops, comm)
        labels = [ids[comm[x]] for x in labels]
        if len(adj) == n_l:
            break
    first: Dict[int, int] = {}
    for v, c in enumerate(labels):
        first.setdefault(c, v)
    return [first[c] for c in labels]


def build(n: int, edges, weights=None, loops=None):
    """One level's graph from its lists -> (adj, loops, k, m2): unique pairs 0 <= i < j < n, a weight per pair (1 where None),
    a loop weight per vertex (0 where None)."""
    adj: List[Dict[int, int]] = [dict() for _ in range(n)]
    for e, (a, b) in enumerate(edges):
        a, b = int(a), int(b)
        assert 0 <= a < b < n and b not in adj[a], (a, b)
        adj[a][b] = adj[b][a] = 1 if weights is None else int(weights[e])
    lp = [0] * n if loops is None else [int(x) for x in loops]
    assert len(lp) == n
    k = [sum(adj[v].values()) + 2 * lp[v] for v in range(n)]
    return adj, lp, k, sum(k)


def degree_classes(adj, limits) -> List[List[int]]:
    """The vertices by number of neighbours: class b holds those with limits[b - 1] < deg <= limits[b] (limits ascending, one
    class more than limits: the last is unbounded), each ascending.  A vertex without a neighbour is in none."""
    out: List[List[int]] = [[] for _ in range(len(limits) + 1)]
    for v, row in enumerate(adj):
        if row:
            out[sum(len(row) > lim for lim in limits)].append(v)
    return out


# ---- numpy forms, for inputs of a million edges: each is held to the Python integers above in tests/test_louvain_ref_host.py ----
def arrays_of(adj):
    """The adjacency as int64 arrays (src, dst, w): every edge from both ends, by (src, dst) ascending."""
    import numpy as np

    src = [v for v, row in enumerate(adj) for _ in row]
    dst = [u for row in adj for u in sorted(row)]
    w = [row[u] for row in adj for u in sorted(row)]
    return np.asarray(src, np.int64), np.asarray(dst, np.int64), np.asarray(w, np.int64)


def csr_np(n: int, pairs, weights=None, loops=None):
    """`build` in numpy -> dict: row_ptr [n + 1], (src, dst, w) by (src, dst) ascending, k, loop, m2 (a Python integer)"""
    import numpy as np

    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    assert ((0 <= p[:, 0]) & (p[:, 0] < p[:, 1]) & (p[:, 1] < n)).all()
    key = p[:, 0] * n + p[:, 1]
    assert len(np.unique(key)) == len(key)
    wt = np.ones(len(p), np.int64) if weights is None else np.asarray(weights, np.int64)
    lp = np.zeros(n, np.int64) if loops is None else np.asarray(loops, np.int64)
    src, dst, w = np.concatenate([p[:, 0], p[:, 1]]), np.concatenate([p[:, 1], p[:, 0]]), np.concatenate([wt, wt])
    order = np.lexsort((dst, src))
    src, dst, w = src[order], dst[order], w[order]
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    k = np.zeros(n, np.int64)
    np.add.at(k, src, w)
    k += 2 * lp
    return {"row_ptr": row_ptr, "src": src, "dst": dst, "w": w, "k": k, "loop": lp, "m2": int(k.sum())}


def quality_np(src, dst, w, loops, k, m2: int, comm) -> int:
    """`quality` over the arrays of `arrays_of` / `csr_np`; every sum stays below 2^63 for m < 2^30 and is taken in int64"""
    import numpy as np

    comm = np.asarray(comm, np.int64)
    tot = np.zeros(len(comm), np.int64)
    np.add.at(tot, comm, np.asarray(k, np.int64))
    inside = int(w[comm[src] == comm[dst]].sum()) + 2 * int(np.asarray(loops, np.int64).sum())
    return int(m2) * inside - int((tot * tot).sum())


def sweep_np(src, dst, w, k, m2: int, comm, t: int):
    """`sweep` over the arrays: (new labels, moved, targets)"""
    import numpy as np

    comm, k = np.asarray(comm, np.int64), np.asarray(k, np.int64)
    n = len(comm)
    tot = np.zeros(n, np.int64)
    np.add.at(tot, comm, k)
    size = np.bincount(comm, minlength=n)
    mover = ((((np.arange(n, dtype=np.uint64) * np.uint64(HASH)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16 + t % 16)) & np.uint64(1)) == 0
    sel = mover[src]
    key, inv = np.unique(src[sel] * n + comm[dst[sel]], return_inverse=True)      # one entry per (mover, neighbouring label)
    w_c = np.zeros(len(key), np.int64)
    np.add.at(w_c, inv.ravel(), w[sel])
    v, c = key // n, key % n
    a = comm[v]
    w_a = np.zeros(n, np.int64)
    w_a[v[c == a]] = w_c[c == a]
    g = int(m2) * (w_c - w_a[v]) - k[v] * (tot[c] - (tot[a] - k[v]))
    cand = (c != a) & (g > 0)
    v, c, g = v[cand], c[cand], g[cand]
    order = np.lexsort((c, -g, v))                                               # per mover: the largest G, then the smallest label
    v, c = v[order], c[order]
    first = np.ones(len(v), bool)
    first[1:] = v[1:] != v[:-1]
    v, c = v[first], c[first]
    go = ~((size[comm[v]] == 1) & (size[c] == 1) & (c > comm[v]))
    new = comm.copy()
    new[v[go]] = c[go]
    return new, int(go.sum()), len(v)


def aggregate_np(src, dst, w, loops, comm):
    """`aggregate` over the arrays -> (n_c, the pairs (a, b, weight) with a < b by (a, b) ascending, new loops, ids [n]: label ->
    new vertex, -1 for a label without members)"""
    import numpy as np

    comm = np.asarray(comm, np.int64)
    n = len(comm)
    used = np.bincount(comm, minlength=n) > 0
    ids = np.where(used, np.cumsum(used) - 1, -1)
    n_c = int(used.sum())
    once = src < dst
    a, b, ww = ids[comm[src[once]]], ids[comm[dst[once]]], w[once]
    nloops = np.zeros(n_c, np.int64)
    np.add.at(nloops, ids[comm], np.asarray(loops, np.int64))
    np.add.at(nloops, a[a == b], ww[a == b])
    out = a != b
    lo, hi = np.minimum(a[out], b[out]), np.maximum(a[out], b[out])
    key, inv = np.unique(lo * n_c + hi, return_inverse=True)
    pw = np.zeros(len(key), np.int64)
    np.add.at(pw, inv.ravel(), ww[out])
    return n_c, (key // n_c, key % n_c, pw), nloops, ids


def levels_run(trace: list) -> int:
    return sum(1 for e in trace if e[0] == "level")


def quality_of_labels(n: int, edges, labels) -> Tuple[int, int]:
    """(Qn, M2) of a labelling of the ORIGINAL graph: modularity = Qn / M2^2."""
    k = [0] * n
    inside = 0
    for a, b in edges:
        k[a] += 1
        k[b] += 1
        if labels[a] == labels[b]:
            inside += 2
    m2 = sum(k)
    tot: Dict[int, int] = {}
    for v in range(n):
        tot[labels[v]] = tot.get(labels[v], 0) + k[v]
    return m2 * inside - sum(t * t for t in tot.values()), m2


def clusters_from_labels(labels, min_size: int = 2) -> List[List[int]]:
    """Communities of at least min_size members, each ascending, ordered by (size descending, smallest member ascending)."""
    groups: Dict[int, List[int]] = {}
    for v, c in enumerate(labels):
        groups.setdefault(int(c), []).append(v)
    return sorted((g for g in groups.values() if len(g) >= min_size), key=lambda g: (-len(g), g[0]))


# ---- inputs shared by the host and the GPU tests (plain python: no networkx needed) ---------------------------------------------
def path_graph(n: int):
    return [(i, i + 1) for i in range(n - 1)]


def cycle_graph(n: int):
    return sorted(path_graph(n) + [(0, n - 1)])


def clique(lo: int, size: int):
    return [(lo + i, lo + j) for i in range(size) for j in range(i + 1, size)]


def disjoint_cliques(sizes):
    edges, lo = [], 0
    for s in sizes:
        edges += clique(lo, s)
        lo += s
    return lo, edges


def ring_of_cliques(n_cliques: int, size: int):
    """networkx.ring_of_cliques with its numbering: vertex 1 of clique q is joined to vertex 0 of clique q + 1."""
    n, edges = disjoint_cliques([size] * n_cliques)
    for q in range(n_cliques):
        a, b = q * size + 1, (q + 1) * size % n
        edges.append((a, b) if a < b else (b, a))
    return n, sorted(set(edges))


def grid_graph(rows: int, cols: int):
    edges = []
    for r in range(rows):
        for c in range(cols):
            v = r * cols + c
            if c + 1 < cols:
                edges.append((v, v + 1))
            if r + 1 < rows:
                edges.append((v, v + cols))
    return rows * cols, edges


def complete_bipartite(a: int, b: int):
    return a + b, [(i, a + j) for i in range(a) for j in range(b)]


def star_and_triangles(leaves: int, triangles: int):
    """hub 0 with `leaves` leaves, then `triangles` disjoint triangles"""
    edges = [(0, 1 + i) for i in range(leaves)]
    lo = 1 + leaves
    for t in range(triangles):
        edges += clique(lo + 3 * t, 3)
    return lo + 3 * triangles, edges
