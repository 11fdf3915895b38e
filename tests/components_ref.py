"""Connected components as csrc/components.hip defines them, in numpy: the synchronous hook-and-jump rule, round
by round, and a plain union-find to hold it against.

    p[v] = v
    a round, from a star forest (every p[v] is a root):
      hook   for every adjacency entry (u, v), with ru = p[u], rv = p[v] as they stood at the start of the round and rv < ru:
             p[ru] = min(p[ru], rv)
      jump   every vertex follows p to its root and stores it
      the round reports whether any hook lowered a parent; the first round that reports none is the last
    label(v) = p[v], the smallest vertex of v's component

The state after every round is a function of the graph alone, so the number of rounds is part of the answer.  From the labels:
n_components, dense[v] = the rank of label(v) among the distinct labels, sizes by dense id, and the largest component, among
equals the one of the smallest label."""
import numpy as np


def round_bound(n):
    """ceil(log2 n) + 2"""
    return max(int(n) - 1, 0).bit_length() + 2


def _entries(n, edges):
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    assert e.size == 0 or (e.min() >= 0 and e.max() < n)
    return np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])


def one_round(p, src, dst):
    """-> (the parents after one hook and jump, whether a hook lowered a parent)"""
    ru, rv = p[src], p[dst]
    hook = rv < ru
    q = p.copy()
    np.minimum.at(q, ru[hook], rv[hook])
    changed = bool(hook.any())
    while True:                                  # the jump: to the root, by doubling
        nxt = q[q]
        if np.array_equal(nxt, q):
            break
        q = nxt
    return q, changed


def rounds_of(n, edges):
    """-> the list of parent arrays, one per round, the last round (which changed nothing) included"""
    src, dst = _entries(n, edges)
    p = np.arange(n, dtype=np.int64)
    states = []
    while True:
        p, changed = one_round(p, src, dst)
        states.append(p)
        if not changed:
            return states


def summarise(labels):
    """labels -> (dense int32 [n], sizes int64 [n_components], n_components, (label, size) of the largest)"""
    labels = np.asarray(labels, dtype=np.int64)
    uniq, dense, sizes = np.unique(labels, return_inverse=True, return_counts=True)
    if uniq.size == 0:
        return dense.astype(np.int32), sizes.astype(np.int64), 0, (-1, 0)
    big = int(np.argmax(sizes))                  # the first maximum: the smallest label among equals
    return dense.reshape(-1).astype(np.int32), sizes.astype(np.int64), int(uniq.size), (int(uniq[big]), int(sizes[big]))


def components(n, edges):
    """-> dict(labels, dense, sizes, n_components, largest, rounds) by the rule; an edgeless graph takes 0 rounds, as
    graph_db.connected_components answers it without a launch"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    if e.shape[0] == 0:
        labels, rounds = np.arange(n, dtype=np.int64), 0
    else:
        states = rounds_of(n, e)
        labels, rounds = states[-1], len(states)
    dense, sizes, n_c, largest = summarise(labels)
    return {"labels": labels, "dense": dense, "sizes": sizes, "n_components": n_c, "largest": largest, "rounds": rounds}


def union_find(n, edges):
    """labels by a plain union-find with path halving: the smallest vertex of each class"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)    # the smaller root stays: a root is the smallest member of its class
    return np.array([find(v) for v in range(n)], dtype=np.int64)


def label_propagation_rounds(n, edges, limit):
    """what the path test is there to fail: rounds of label(v) = min over v and its neighbours, until nothing changes (cut at
    `limit`)"""
    src, dst = _entries(n, edges)
    lab = np.arange(n, dtype=np.int64)
    for r in range(1, limit + 1):
        nxt = lab.copy()
        np.minimum.at(nxt, src, lab[dst])
        if np.array_equal(nxt, lab):
            return r
        lab = nxt
    return limit


# ---- graphs --------------------------------------------------------------------------------------------------------------------------
def scrambled_path(n, seed):
    """a path of n vertices under a fixed random renumbering"""
    perm = np.random.default_rng(seed).permutation(n)
    return np.stack([perm[:-1], perm[1:]], axis=1)


def star_clique_isolated(leaves=8200, clique=70, isolated=50):
    """hub 0 with `leaves` leaves, then a clique, then vertices without an edge: degrees 1, clique - 1, leaves and 0"""
    star = [(0, i) for i in range(1, leaves + 1)]
    c0 = leaves + 1
    k = [(c0 + i, c0 + j) for i in range(clique) for j in range(i + 1, clique)]
    return leaves + 1 + clique + isolated, np.array(star + k, dtype=np.int64)


def caterpillar_of_stars(stars=64, leaves=64):
    """`stars` stars of `leaves` leaves whose hubs form a path: hub s is vertex s * (leaves + 1) + leaves, the LARGEST vertex of
    its star and smaller than everything in star s + 1, so in the first round hub s + 1 hooks to hub s, hub s to hub s - 1, ..,
    hub 0 to vertex 0 — one chain of `stars` hooks, down the ids, for a single jump pass"""
    edges, hubs = [], []
    for s in range(stars):
        base = s * (leaves + 1)
        hub = base + leaves
        hubs.append(hub)
        edges += [(base + i, hub) for i in range(leaves)]
    edges += [(hubs[s], hubs[s + 1]) for s in range(stars - 1)]
    return stars * (leaves + 1), np.array(edges, dtype=np.int64)


def random_sparse(n, m, seed):
    """m distinct pairs i < j, uniformly"""
    rng = np.random.default_rng(seed)
    got = np.zeros((0, 2), np.int64)
    while got.shape[0] < m:
        e = rng.integers(0, n, (2 * (m - got.shape[0]) + 16, 2), dtype=np.int64)
        e = e[e[:, 0] != e[:, 1]]
        got = np.unique(np.concatenate([got, np.stack([e.min(axis=1), e.max(axis=1)], axis=1)]), axis=0)
    return got[rng.permutation(got.shape[0])[:m]]


def chain_embeddings(lengths=(3, 4, 5, 6, 3, 6, 4, 5, 6, 6), seed=2):
    """the chains case of tests/test_gpu_louvain.py, rebuilt: chains A ~ B ~ C with A !~ C at 0.95 — consecutive rows 15 degrees
    apart (cosine 0.966), rows two steps apart 30 degrees (0.866), each chain in a plane of its own, the rows shuffled.
    -> (float32 [rows][2 * chains], the chain of each row, the pairs (i < j) of consecutive rows of a chain)"""
    rows, chain = [], []
    for c, length in enumerate(lengths):
        for s in range(length):
            v = np.zeros(2 * len(lengths))
            v[2 * c], v[2 * c + 1] = np.cos(np.radians(15.0 * s)), np.sin(np.radians(15.0 * s))
            rows.append((1.0 + 0.25 * s) * v)
            chain.append(c)
    perm = np.random.default_rng(seed).permutation(len(rows))
    where = np.argsort(perm)                     # where row r of the unshuffled order went
    pairs, r = [], 0
    for length in lengths:
        pairs += [(min(where[r + s], where[r + s + 1]), max(where[r + s], where[r + s + 1])) for s in range(length - 1)]
        r += length
    return np.asarray(rows)[perm].astype(np.float32), np.asarray(chain)[perm], np.array(sorted(pairs), dtype=np.int64)


def planted_duplicates(n=2000, d=64, seed=11, sizes=(40, 17, 9, 5, 3, 2, 2)):
    """n unit rows of d dimensions: random directions (pairwise cosine far below 0.95 at d = 64), and groups of near-copies of
    one of them (noise 0.01: cosine above 0.99 inside a group) at scattered rows.  -> (float32 [n][d], group int [n], -1 = none)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    group = np.full(n, -1)
    free = rng.permutation(n)
    at = 0
    for g, size in enumerate(sizes):
        rows = free[at:at + size]
        at += size
        x[rows] = x[rows[0]] + 0.01 * rng.standard_normal((size, d)) / np.sqrt(d)
        group[rows] = g
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), group
