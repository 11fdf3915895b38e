"""The five steps of csrc/louvain.hip one at a time — rarc_graph_csr, rarc_louvain_init, _sweep, _aggregate, _labels — called
through the C ABI on torch buffers as communities._cluster_on_device calls them, and everything a step writes read where it
lies (tests/louvain_blob.py) and compared with tests/louvain_ref.py.  Every comparison is exact equality of integers.

tests/test_gpu_louvain.py compares the final labels of the whole driver; what it cannot see and this file does: Qn of every
sweep (the driver only asks q <= best), `targets`, weights and loops in the table forms of the sweep, the aggregate's own
outputs, the GRAPH blob every graph kernel reads, and every scan and grid-stride loop on its second trip (the large case)."""
import collections

import numpy as np
import pytest

from tests import louvain_blob as LB
from tests import louvain_ref as R

pytestmark = pytest.mark.gpu

WEIGHTS = (1, 1, 2, 3, 7, 1000)


def _limits():
    from rag_arc_amd.encapsulation.database.graph_db.communities import bucket_limits

    lim = bucket_limits()
    return [lim["group"], lim["wave"], lim["lds"]]


# ---- the device side: one level's buffers and the calls on them -----------------------------------------------------------------------
def _u32(x):
    """uint32 values below 2^31 as the int32 tensor torch has"""
    import torch

    a = np.asarray(x, np.int64)
    assert a.size == 0 or (0 <= a.min() and a.max() < 1 << 31)
    return torch.from_numpy(a.astype(np.int32)).cuda()


class Level:
    def __init__(self, n, pairs, weights=None, loops=None):
        import torch

        from rag_arc_amd.hip import binding as B

        self.B, self.lib = B, B.load_library()
        p = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
        self.n, self.m = int(n), len(p)
        self.pairs = torch.from_numpy(p).cuda()
        self.w = None if weights is None else _u32(weights)
        self.loops = None if loops is None else _u32(loops)
        assert self.w is None or self.w.numel() == self.m
        assert self.loops is None or self.loops.numel() == self.n
        gb, sb = int(self.lib.rarc_graph_csr_workspace_bytes(self.n, self.m)), int(self.lib.rarc_louvain_workspace_bytes(self.n, self.m))
        assert gb == LB.graph_bytes(self.n, self.m) and sb == LB.state_bytes(self.n, self.m)
        self.graph = torch.zeros(gb, dtype=torch.uint8, device="cuda")
        self.state = torch.zeros(sb, dtype=torch.uint8, device="cuda")
        self.out3 = torch.full((3,), -99, dtype=torch.int64, device="cuda")
        self.stream = torch.cuda.current_stream().cuda_stream
        self.args = (self.graph.data_ptr(), gb, self.n, self.m, self.state.data_ptr(), sb)

    def csr(self):
        ptr = lambda t: None if t is None else t.data_ptr()
        self.B.check(self.lib.rarc_graph_csr(self.pairs.data_ptr(), ptr(self.w), ptr(self.loops), self.n, self.m, self.args[0], self.args[1],
                                             self.stream), "rarc_graph_csr")
        return LB.read_graph(self.graph.cpu().numpy(), self.n, self.m)

    def init(self):
        self.out3.fill_(-99)
        self.B.check(self.lib.rarc_louvain_init(*self.args, self.out3.data_ptr(), self.stream), "rarc_louvain_init")
        return self.out3.tolist()

    def sweep(self, cur, t):
        self.out3.fill_(-99)
        self.B.check(self.lib.rarc_louvain_sweep(*self.args, cur, t, self.out3.data_ptr(), self.stream), "rarc_louvain_sweep")
        return self.out3.tolist()

    def slots(self):
        head = LB.state_offsets(self.n, self.m)[0]["scal"]
        return LB.read_state(self.state[:head].cpu().numpy(), self.n, self.m)

    def aggregate(self, cur, labels):
        """-> (n_c, m_c, pairs [m][2], weights [m], loops [n], labels [n0]) on the host; what the call left unwritten reads -7"""
        import torch

        n0 = len(labels)
        d_labels = torch.from_numpy(np.asarray(labels, np.int64)).cuda()
        o_pairs = torch.full((self.m, 2), -7, dtype=torch.int64, device="cuda")
        o_w = torch.full((self.m,), -7, dtype=torch.int32, device="cuda")
        o_loops = torch.full((self.n,), -7, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), -7, dtype=torch.int64, device="cuda")
        self.B.check(self.lib.rarc_louvain_aggregate(*self.args, cur, d_labels.data_ptr(), n0, o_pairs.data_ptr(), o_w.data_ptr(),
                                                     o_loops.data_ptr(), counts.data_ptr(), self.stream), "rarc_louvain_aggregate")
        n_c, m_c = counts.tolist()
        return n_c, m_c, o_pairs.cpu().numpy(), o_w.cpu().numpy().astype(np.int64), o_loops.cpu().numpy().astype(np.int64), d_labels.cpu().numpy()


def _final_labels(labels):
    import torch

    from rag_arc_amd.hip import binding as B

    lib = B.load_library()
    d = torch.from_numpy(np.asarray(labels, np.int64)).cuda()
    ws = torch.zeros(int(lib.rarc_louvain_labels_workspace_bytes(len(labels))), dtype=torch.uint8, device="cuda")
    B.check(lib.rarc_louvain_labels(d.data_ptr(), len(labels), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream),
            "rarc_louvain_labels")
    return d.cpu().numpy()


# ---- the comparisons ------------------------------------------------------------------------------------------------------------------
def _ref_csr(adj, loops, k, m2):
    """the reference of `R.build` in the arrays of `R.csr_np`"""
    src, dst, w = R.arrays_of(adj)
    row_ptr = np.zeros(len(adj) + 1, np.int64)
    np.cumsum([len(r) for r in adj], out=row_ptr[1:])
    return {"row_ptr": row_ptr, "src": src, "dst": dst, "w": w, "k": np.asarray(k, np.int64), "loop": np.asarray(loops, np.int64), "m2": m2}


def check_csr(G, ref, bad=0):
    """everything rarc_graph_csr wrote against the reference's arrays (R.csr_np's dict)"""
    n = len(ref["k"])
    deg = np.diff(ref["row_ptr"])
    entries = len(ref["src"])
    assert np.array_equal(G["row_ptr"], ref["row_ptr"]) and G["row_ptr"][n] == entries
    assert np.array_equal(G["adj_src"][:entries], np.repeat(np.arange(n), deg))
    adj, adj_w, adj_src = (G[x][:entries].astype(np.int64) for x in ("adj", "adj_w", "adj_src"))
    order = np.lexsort((adj_w, adj, adj_src))                     # a row's entries as a multiset: the order inside a row is free
    assert np.array_equal(adj[order], ref["dst"]) and np.array_equal(adj_w[order], ref["w"])
    assert np.array_equal(G["k"], ref["k"]) and np.array_equal(G["loop"], ref["loop"])
    assert G["hdr"][LB.H_M2] == ref["m2"] == int(ref["k"].sum())
    assert G["hdr"][LB.H_BAD] == bad
    lim = _limits()
    cls = np.where(deg == 0, -1, (deg > lim[0]).astype(int) + (deg > lim[1]) + (deg > lim[2]))
    for b in range(4):
        want = np.nonzero(cls == b)[0]
        assert G["hdr"][LB.H_LIST + b] == len(want), b
        assert np.array_equal(np.sort(G["list"][b][:len(want)]), want), b


def check_slot(S, s, comm, k):
    comm = np.asarray(comm, np.int64)
    assert np.array_equal(S["comm"][s], comm)
    tot = np.zeros(len(comm), np.int64)
    np.add.at(tot, comm, np.asarray(k, np.int64))
    assert np.array_equal(S["tot"][s], tot)                       # zero for a label without members
    assert np.array_equal(S["size"][s], np.bincount(comm, minlength=len(comm)))


def same_slot(S, T, s):
    return all(np.array_equal(S[x][s], T[x][s]) for x in ("comm", "tot", "size"))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def random_pairs(rng, lo, hi, count, taken):
    out = []
    while len(out) < count:
        a, b = int(rng.integers(lo, hi)), int(rng.integers(lo, hi))
        e = (min(a, b), max(a, b))
        if a != b and e not in taken:
            taken.add(e)
            out.append(e)
    return out


def ladder_graph():
    """one vertex of each degree 1, g, g + 1, w, w + 1, l, l + 1 (g, w, l: the limits of the degree classes) over a shared pool of
    l + 1 leaves: the vertex of degree d is joined to the leaves 0 .. d - 1, so a leaf has at most 7 neighbours and at least one"""
    g, w, l = _limits()
    degrees = [1, g, g + 1, w, w + 1, l, l + 1]
    pool = l + 1
    pairs = [(leaf, pool + i) for i, d in enumerate(degrees) for leaf in range(d)]
    return pool + len(degrees), pairs, None, None


def weighted_loops_graph():
    rng = np.random.default_rng(21)
    n = 1200
    pairs = random_pairs(rng, 0, n, 2500, set())
    return n, pairs, rng.choice(WEIGHTS, len(pairs)).tolist(), np.where(rng.random(n) < .3, rng.integers(1, 9, n), 0).tolist()


def salted_pairs():
    """good pairs with one bad pair after every fourth: i == j, i > j, a negative end, j >= n"""
    rng = np.random.default_rng(22)
    n = 50
    good = random_pairs(rng, 0, n, 60, set())
    bad = [(3, 3), (7, 2), (-1, 4), (4, n), (0, 1 << 40), (-5, -2), (n, n + 9), (n - 1, n - 1), (49, 0), (-(1 << 40), 5), (0, 0), (1, n + 1)]
    mixed, weights = [], []
    for i, e in enumerate(good):
        mixed.append(e)
        weights.append(1 + i % 5)
        if i % 4 == 3 and i // 4 < len(bad):
            mixed.append(bad[i // 4])
            weights.append(999)
    assert sum(1 for a, b in mixed if not 0 <= a < b < n) == len(bad) == 12
    return n, mixed, weights, None


HEAVY = (1 << 30) - 1


def hub_graph():
    """about 9,400 vertices and 23,000 weighted edges with loops: designated vertices of every degree class, the last ids, each
    joined to random leaves; the leaves share a sparse random background.  The two largest hubs have one edge of weight 300,000."""
    g, w, l = _limits()
    rng = np.random.default_rng(3)
    degrees = [9, 9, 9, 9, 9, 9, 9, 9, 30, 30, 30, 30, 30, 30, w, w, w, w, w + 1, w + 1, w + 1, w + 1, 300, 300, 300, l, l + 800]
    assert g < 9 and 30 <= w < 300 <= l
    n = 9400
    leaves = n - len(degrees)
    taken = set()
    pairs = random_pairs(rng, 0, leaves, 4200, taken)
    weights = rng.choice(WEIGHTS, len(pairs)).tolist()
    for i, d in enumerate(degrees):
        mine = rng.choice(leaves, d, replace=False)
        pairs += [(int(u), leaves + i) for u in mine]
        weights += rng.choice(WEIGHTS, d).tolist()
        if d >= l:
            weights[-1] = 300_000
    order = rng.permutation(len(pairs))
    loops = np.where(rng.random(n) < .25, rng.integers(1, 6, n), 0)
    return n, [pairs[i] for i in order], [weights[i] for i in order], loops.tolist()


def loops_everywhere_graph():
    """the shape of a level >= 1: few vertices, heavy weights, a loop on every vertex"""
    rng = np.random.default_rng(23)
    n = 40
    pairs = random_pairs(rng, 0, n, 110, set())
    return n, pairs, rng.integers(1, 60, len(pairs)).tolist(), rng.integers(1, 400, n).tolist()


GRAPHS = {
    "edge": lambda: (2, [(0, 1)], None, None),
    "ladder": ladder_graph,
    "weighted-loops": weighted_loops_graph,
    "salted": salted_pairs,
    "heavy-edge": lambda: (2, [(0, 1)], [HEAVY], None),
    "hub": hub_graph,
    "k30-30": lambda: R.complete_bipartite(30, 30) + (None, None),
    "clique600": lambda: (600, R.clique(0, 600), None, None),
    "loops-everywhere": loops_everywhere_graph,
}


class Ref:
    """One input and the reference's answers on it, computed once per session and never modified."""

    def __init__(self, name):
        self.n, self.given, self.given_w, self.loops_in = GRAPHS[name]()
        keep = [i for i, (a, b) in enumerate(self.given) if 0 <= a < b < self.n]
        self.bad = len(self.given) - len(keep)
        self.adj, self.loops, self.k, self.m2 = R.build(self.n, [self.given[i] for i in keep],
                                                        None if self.given_w is None else [self.given_w[i] for i in keep], self.loops_in)
        self.q0 = R.quality(self.adj, self.loops, self.k, self.m2, list(range(self.n)))
        self._kept, self._from = None, {}

    def level(self):
        return Level(self.n, self.given, self.given_w, self.loops_in)

    def step(self, comm, t):
        new, moved, targets = R.sweep(self.adj, self.loops, self.k, self.m2, comm, t)
        return new, moved, R.quality(self.adj, self.loops, self.k, self.m2, new), targets

    def kept(self):
        """state[t] = the labels before sweep t when every sweep is kept, t = 0 .. 8; out[t] = (moved, Qn, targets) of sweep t"""
        if self._kept is None:
            state, out = [list(range(self.n))], []
            for t in range(8):
                new, moved, q, targets = self.step(state[-1], t)
                state.append(new)
                out.append((moved, q, targets))
            self._kept = (state, out)
        return self._kept

    def step_from(self, start, t):
        """sweep t of the state after `start` kept sweeps (the same answer for every t with the same t mod 16: only it selects)"""
        if (start, t % 16) not in self._from:
            self._from[start, t % 16] = self.step(self.kept()[0][start], t % 16)
        return self._from[start, t % 16]


_REFS = {}


def ref_of(name) -> Ref:
    if name not in _REFS:
        _REFS[name] = Ref(name)
    return _REFS[name]


# ---- the adjacency --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge", "ladder", "weighted-loops", "salted", "heavy-edge", "hub"])
def test_csr(name):
    ref = ref_of(name)
    lev = ref.level()
    G = lev.csr()
    check_csr(G, _ref_csr(ref.adj, ref.loops, ref.k, ref.m2), bad=ref.bad)
    deg = sorted(len(r) for r in ref.adj)
    if name == "ladder":
        g, w, l = _limits()
        assert [d for d in deg if d > g - 1] == [g, g + 1, w, w + 1, l, l + 1] and deg.count(0) == 0 and ref.n < l + 10
    if name == "salted":
        assert ref.bad == 12 and G["row_ptr"][ref.n] == 2 * (lev.m - 12)
    if name == "heavy-edge":
        assert ref.m2 == (1 << 31) - 2 and ref.q0 == -2 * HEAVY ** 2
    if name == "weighted-loops":
        assert any(ref.loops) and len(set(w for r in ref.adj for w in r.values())) == 5 and deg[0] == 0


# ---- init, sweep and evaluation -------------------------------------------------------------------------------------------------------
SWEEP_GRAPHS = ["hub", "k30-30", "edge", "heavy-edge", "clique600", "loops-everywhere"]


def _w_own(ref, comm, v):
    return sum(w for u, w in ref.adj[v].items() if comm[u] == comm[v])


def _input_conditions(name, ref):
    """what each input is there for, asserted from the reference alone"""
    state, out = ref.kept()
    if name == "hub":
        # every degree class has, within the eight kept sweeps, a mover that moves and a mover that sits in a community of at
        # least two members and has an edge into it (w_A > 0)
        classes = R.degree_classes(ref.adj, _limits())
        moves, sits = [0] * 4, [0] * 4
        for t in range(8):
            size = collections.Counter(state[t])
            for b, members in enumerate(classes):
                for v in members:
                    if R.is_mover(v, t):
                        moves[b] += state[t + 1][v] != state[t][v]
                        sits[b] += size[state[t][v]] >= 2 and _w_own(ref, state[t], v) > 0
        assert all(moves) and all(sits), (moves, sits)
        deg = [len(r) for r in ref.adj]
        g, w, l = _limits()
        assert max(deg) > l + 500 and {l, 300, w + 1, w, 30, 9} <= set(deg) and 9000 < ref.n < 9800
        assert sum(1 for x in ref.loops if x) > ref.n // 5 and len(set(x for r in ref.adj for x in r.values())) == 6
        assert [len(c) for c in classes][1:] == [18, 8, 1]
    if name == "k30-30":
        assert out[0][0] > 0 and out[0][1] < ref.q0             # the overshoot: the one discard the driver knows
    if name in ("edge", "heavy-edge"):
        # vertex 0 is held back by the singleton rule until vertex 1 is a mover: nothing moves, yet a mover has a target
        assert [(o[0], o[2]) for o in out[:4]] == [(0, 1), (0, 1), (0, 1), (1, 2)] and out[3][1] == 0 and out[0][1] == ref.q0
    if name == "clique600":
        g, w, l = _limits()
        assert w < 599 <= l and out[0][0] > 0
    if name == "loops-everywhere":
        assert all(ref.loops) and any(o[0] for o in out)


@pytest.mark.parametrize("name", SWEEP_GRAPHS)
def test_every_sweep_kept(name):
    """init, then sweeps 0 .. 7, each kept whether Qn rose or not: states the driver never reaches, and Qn there is still Qn"""
    ref = ref_of(name)
    _input_conditions(name, ref)
    state, out = ref.kept()
    lev = ref.level()
    lev.csr()
    assert lev.init() == [0, ref.q0, 0]
    S = lev.slots()
    check_slot(S, 0, state[0], ref.k)
    cur = 0
    for t in range(8):
        got = lev.sweep(cur, t)
        T = lev.slots()
        moved, q, targets = out[t]
        assert got == [moved, q, targets], t
        check_slot(T, cur ^ 1, state[t + 1], ref.k)
        assert same_slot(S, T, cur), t                          # the slot that was read
        S, cur = T, cur ^ 1


@pytest.mark.parametrize("start", [0, 2])
@pytest.mark.parametrize("name", SWEEP_GRAPHS)
def test_sweeps_discarded(name, start):
    """From the state after `start` kept sweeps, sweeps without a flip between them: each is the reference's sweep of that same
    state, and only t mod 16 selects the movers."""
    ref = ref_of(name)
    state, _ = ref.kept()
    lev = ref.level()
    lev.csr()
    lev.init()
    cur = 0
    for t in range(start):
        lev.sweep(cur, t)
        cur ^= 1
    S = lev.slots()
    check_slot(S, cur, state[start], ref.k)
    seen = {}
    for t in (start, start + 1, 0, 16, 1 << 20):
        got = lev.sweep(cur, t)
        T = lev.slots()
        new, moved, q, targets = ref.step_from(start, t)
        assert got == [moved, q, targets], t
        check_slot(T, cur ^ 1, new, ref.k)
        assert same_slot(S, T, cur), t
        seen[t] = (got, T["comm"][cur ^ 1].copy())
    for t in (16, 1 << 20):
        assert seen[t][0] == seen[0][0] and np.array_equal(seen[t][1], seen[0][1])


# ---- the aggregate --------------------------------------------------------------------------------------------------------------------
def _labels_in(n, n0, rng):
    """a map into [0, n) that is not the identity, and four entries outside it"""
    labels = rng.integers(0, n, n0)
    outside = {5: -1, 100: n + 5, 7: 1 << 40, n0 - 1: n}
    for i, x in outside.items():
        labels[i] = x
    return labels, outside


@pytest.mark.parametrize("sweeps", [0, 1, 3, 8])
def test_aggregate_of_the_hub_graph(sweeps):
    ref = ref_of("hub")
    comm = ref.kept()[0][sweeps]
    nadj, nloops, ids = R.aggregate(ref.adj, ref.loops, comm)
    want_pairs = {(a, b): w for a in range(len(nadj)) for b, w in nadj[a].items() if a < b}
    assert (len(nadj) == ref.n) == (sweeps == 0) and len(nadj) >= 2 and want_pairs
    lev = ref.level()
    lev.csr()
    lev.init()
    cur = 0
    for t in range(sweeps):
        lev.sweep(cur, t)
        cur ^= 1
    labels, outside = _labels_in(ref.n, ref.n + 37, np.random.default_rng(sweeps))
    n_c, m_c, pairs, weights, loops, composed = lev.aggregate(cur, labels)
    assert (n_c, m_c) == (len(nadj), len(want_pairs))
    got_pairs = {(int(a), int(b)): int(w) for (a, b), w in zip(pairs[:m_c], weights[:m_c])}
    assert len(got_pairs) == m_c and got_pairs == want_pairs       # no pair twice, every pair a < b (the reference's keys)
    assert loops[:n_c].tolist() == nloops
    for i, x in enumerate(labels):
        assert composed[i] == (x if i in outside else ids[comm[x]]), i     # ids: ascending label order
    # aggregation conserves the total weight: the next level's CSR from these outputs
    nxt = Level(n_c, pairs[:m_c], weights[:m_c], loops[:n_c])
    nk = [sum(nadj[v].values()) + 2 * nloops[v] for v in range(n_c)]
    assert sum(nk) == ref.m2
    check_csr(nxt.csr(), _ref_csr(nadj, nloops, nk, ref.m2))


# ---- the final labels -----------------------------------------------------------------------------------------------------------------
def _smallest_member(labels):
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    return first[inv.ravel()]


LABELLINGS = {
    "random": lambda: np.random.default_rng(31).integers(0, 5000, 5000),
    "few-classes": lambda: np.random.default_rng(32).integers(4000, 4010, 5000),
    "constant": lambda: np.full(3000, 2999),
    "reversed": lambda: np.arange(3000)[::-1].copy(),
    "one": lambda: np.zeros(1, np.int64),
    "second-trip": lambda: np.random.default_rng(33).integers(0, 524_288 + 5, 524_288 + 5),
}


@pytest.mark.parametrize("name", list(LABELLINGS))
def test_labels_are_the_smallest_member(name):
    """any labelling with values in [0, n0), not only the driver's"""
    labels = LABELLINGS[name]()
    want = _smallest_member(labels)
    if name == "constant":
        assert want.tolist() == [0] * 3000
    if name == "reversed":
        assert want.tolist() == list(range(3000))
    if name == "second-trip":
        assert len(labels) > 2048 * 256 and (want[2048 * 256:] != np.arange(2048 * 256, len(labels))).any()
    assert np.array_equal(_final_labels(labels), want)


# ---- the large case: every scan and every grid-stride loop on its second trip ---------------------------------------------------------
LARGE_N = 257 * LB.SCAN_TILE + 3
PLANTED = (2047, 2048, 524_287, 524_288, LARGE_N - 1)


@pytest.fixture(scope="module")
def large():
    """n = 526,339 (257 full scan tiles and 3 vertices: the offsets kernel's second pass is partial), a little over 2^20 unique
    random pairs on half of the vertices, weights and loops.  The references are the numpy forms, which
    tests/test_louvain_ref_host.py holds to the Python integers; the device calls are made here once and the tests read."""
    n = LARGE_N
    rng = np.random.default_rng(41)
    active = np.union1d(rng.choice(n, n // 2, replace=False), PLANTED)
    draw = np.sort(active[rng.integers(0, len(active), (1_060_000, 2))], axis=1)
    extra = np.asarray([(min(v, u), max(v, u)) for v in PLANTED for u in (active[0], active[1])])
    draw = np.concatenate([draw, extra])
    draw = draw[draw[:, 0] != draw[:, 1]]
    _, first = np.unique(draw[:, 0] * n + draw[:, 1], return_index=True)
    pairs = draw[np.sort(first)]                                   # unique, in the order drawn
    weights = rng.choice(WEIGHTS, len(pairs))
    loops = np.where(rng.random(n) < .25, rng.integers(1, 6, n), 0)
    c = R.csr_np(n, pairs, weights, loops)
    deg = np.diff(c["row_ptr"])
    # what the case is there for
    # (the offsets kernel scans 256 tile sums per pass: 258 tiles make a second pass of two, the last tile 3 vertices long)
    assert len(pairs) > 1 << 20 and 256 < LB.scan_blocks(n) == 258 < 512 and n % LB.SCAN_TILE == 3 and n > 2048 * 256
    assert .4 < (deg == 0).mean() < .6 and all(deg[v] > 0 for v in PLANTED) and c["m2"] < 1 << 31
    ident = np.arange(n)
    out = {"n": n, "pairs": pairs, "csr": c, "q0": R.quality_np(c["src"], c["dst"], c["w"], c["loop"], c["k"], c["m2"], ident)}
    new, moved, targets = R.sweep_np(c["src"], c["dst"], c["w"], c["k"], c["m2"], ident, 0)
    out["sweep"] = (new, [moved, R.quality_np(c["src"], c["dst"], c["w"], c["loop"], c["k"], c["m2"], new), targets])
    assert moved > 1000 and len(np.unique(new[2048 * 256:])) > 1
    out["aggregate"] = R.aggregate_np(c["src"], c["dst"], c["w"], c["loop"], new)
    lev = Level(n, pairs, weights, loops)
    out["G"] = lev.csr()
    out["init"] = lev.init()
    out["S0"] = lev.slots()
    out["swept"] = lev.sweep(0, 0)
    out["S1"] = lev.slots()
    out["labels"], out["outside"] = _labels_in(n, n + 37, rng)
    out["agg"] = lev.aggregate(1, out["labels"])
    out["S2"] = lev.slots()
    return out


def test_large_csr(large):
    check_csr(large["G"], large["csr"])


def test_large_init_and_sweep(large):
    c = large["csr"]
    assert large["init"] == [0, large["q0"], 0]
    check_slot(large["S0"], 0, np.arange(large["n"]), c["k"])
    new, words = large["sweep"]
    assert large["swept"] == words
    check_slot(large["S1"], 1, new, c["k"])
    assert same_slot(large["S0"], large["S1"], 0)


def test_large_aggregate(large):
    n = large["n"]
    new = large["sweep"][0]
    want_n, (wa, wb, ww), want_loops, ids = large["aggregate"]
    n_c, m_c, pairs, weights, loops, composed = large["agg"]
    assert (n_c, m_c) == (want_n, len(wa)) and n_c < n
    a, b = pairs[:m_c, 0], pairs[:m_c, 1]
    assert (a < b).all()
    order = np.lexsort((b, a))
    assert np.array_equal(a[order], wa) and np.array_equal(b[order], wb) and np.array_equal(weights[:m_c][order], ww)   # so no pair twice
    assert np.array_equal(loops[:n_c], want_loops)
    labels, outside = large["labels"], large["outside"]
    want = labels.copy()
    inside = np.ones(len(labels), bool)
    inside[list(outside)] = False
    want[inside] = ids[new[labels[inside]]]
    assert np.array_equal(composed, want)
    assert same_slot(large["S1"], large["S2"], 0) and same_slot(large["S1"], large["S2"], 1)       # the aggregate only reads the labels
