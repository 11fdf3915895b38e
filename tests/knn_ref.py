"""The oracle, the comparison and the seeded inputs of the knn_graph tests (tests/test_knn_ref_host.py on the CPU,
tests/test_gpu_knn_graph.py and tests/test_gpu_self_join_lists.py on the GPU).  Plain numpy.

The arithmetic is the one oracle/cpu_ref.py: similar_pairs_f64 restates from scikit-learn's cosine_similarity (the function the
reference calls for its other self-join): rows divided by their float64 norms, zero rows left alone, then xn @ xn.T.  A kNN graph
(event_graphrag_neo4j.py:636-649: gds.knn.write, topK, similarityCutoff) is, per row, the other rows with cosine >= cutoff
ordered by (cosine desc, index asc) and cut at top_k."""
import numpy as np

BAND = 1e-12      # two float64 summation orders of one dot product (tests/test_gpu_similar_pairs.py uses the same band)


def cosine_matrix_f64(x):
    x = np.asarray(x, dtype=np.float64)
    norms = np.sqrt(np.einsum("ij,ij->i", x, x))
    norms[norms == 0.0] = 1.0                       # sklearn.preprocessing.normalize: zero rows are left alone
    xn = x / norms[:, None]
    return xn @ xn.T


def _bars(sim, top_k, cutoff):
    """(S, bar, nxt): S = sim with the diagonal at -inf (self goes by index); bar[i] = max(cutoff, the top_k-th largest cosine of
    row i's others) — the cutoff where there are fewer than top_k others; nxt[i] = max(cutoff, the (top_k + 1)-th largest)."""
    n = sim.shape[0]
    S = sim.copy()
    S[np.arange(n), np.arange(n)] = -np.inf
    bar = np.full(n, float(cutoff))
    nxt = np.full(n, float(cutoff))
    if n - 1 >= top_k:
        part = np.partition(S, [n - top_k - 1, n - top_k], axis=1)     # (column n - top_k - 1 >= 0 holds the diagonal's -inf at worst)
        bar = np.maximum(bar, part[:, n - top_k])
        nxt = np.maximum(nxt, part[:, n - top_k - 1])
    return S, bar, nxt


def _must_may(S, bar, nxt, band):
    """must: beats the cutoff and the (top_k + 1)-th best by more than the band — in the answer whichever way float64 noise falls;
    may: within the band of the cutoff and of the top_k-th best, or better.  (Every j with cosine > max(kth, cutoff) + band is in
    must, and the top_k-th best itself is too wherever the next one lies further than the band under it: then may == must.)"""
    return S > (nxt + band)[:, None], S >= (bar - band)[:, None]


def knn_from_sim(sim, top_k, cutoff):
    """(ids int64 [n][top_k], cosines float64 [n][top_k], counts int32 [n]) from a cosine matrix; the diagonal goes by index."""
    n = sim.shape[0]
    ids = np.full((n, top_k), -1, np.int64)
    cos = np.full((n, top_k), -np.inf, np.float64)
    cnt = np.zeros(n, np.int32)
    S, bar, _ = _bars(sim, top_k, cutoff)
    for i in range(n):
        row = S[i]
        j = np.nonzero(row >= bar[i])[0]            # the answer and whatever ties with its last entry
        j = j[np.lexsort((j, -row[j]))][:top_k]     # (cosine desc, j asc)
        ids[i, :len(j)] = j
        cos[i, :len(j)] = row[j]
        cnt[i] = len(j)
    return ids, cos, cnt


def knn_graph_f64(x, top_k, cutoff):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2:
        n = x.shape[0] if x.ndim == 2 else 0
        return np.full((n, top_k), -1, np.int64), np.full((n, top_k), -np.inf, np.float64), np.zeros(n, np.int32)
    return knn_from_sim(cosine_matrix_f64(x), top_k, cutoff)


def band_rows(sim, top_k, cutoff, band=BAND):
    """How many rows have an answer the band could excuse anything in (may != must; must is a subset of may)."""
    must, may = _must_may(*_bars(sim, top_k, cutoff), band)
    return int((must != may).any(axis=1).sum())


def min_gap_in_answers(want):
    """The smallest difference between consecutive cosines of any row's oracle answer: above the float64 noise, the order of
    the ids is decided by the cosines alone."""
    _, cos, cnt = want
    with np.errstate(invalid="ignore"):             # (padding: -inf - -inf, masked out below)
        gaps = cos[:, :-1] - cos[:, 1:]
    live = np.arange(cos.shape[1] - 1)[None, :] < (cnt[:, None] - 1)
    return float(gaps[live].min()) if live.any() else np.inf


def compare(got, sim, top_k, cutoff, band=BAND, what=""):
    """got = (ids, cosines, counts) as knn_graph(..., as_arrays=True) returns them; sim the oracle's cosine matrix."""
    ids, cos, cnt = got
    n = sim.shape[0]
    all_must, all_may = _must_may(*_bars(sim, top_k, cutoff), band)
    assert ids.shape == (n, top_k) and cos.shape == (n, top_k) and cnt.shape == (n,), (what, ids.shape, cos.shape, cnt.shape)
    assert ids.dtype == np.int64 and cos.dtype == np.float64 and cnt.dtype == np.int32, what
    for i in range(n):
        c = int(cnt[i])
        must = set(np.nonzero(all_must[i])[0].tolist())
        may = set(np.nonzero(all_may[i])[0].tolist())
        g = ids[i, :c].tolist()
        gs = cos[i, :c]
        assert 0 <= c <= top_k, (what, i, c)
        assert np.all(ids[i, c:] == -1) and np.all(np.isneginf(cos[i, c:])), (what, i, "padding")
        assert len(set(g)) == c and i not in g and all(0 <= j < n for j in g), (what, i, g)
        assert must <= set(g) <= may, (what, i, sorted(must - set(g)), sorted(set(g) - may))
        assert min(top_k, len(must)) <= c <= min(top_k, len(may)), (what, i, c, len(must), len(may))
        if c:
            assert np.max(np.abs(gs - sim[i, g])) <= 1e-12, (what, i, "scores")
            order = np.lexsort((np.asarray(g), -gs))
            assert np.array_equal(order, np.arange(c)), (what, i, "not ordered by (score desc, j asc)")


def assert_equal_in_order(got, want, what=""):
    """The exact category: ids equal the oracle's in order, counts equal, scores within 1e-12."""
    ids, cos, cnt = got
    w_ids, w_cos, w_cnt = want
    assert np.array_equal(cnt, w_cnt), (what, "counts", np.nonzero(cnt != w_cnt)[0][:8])
    bad = np.nonzero((ids != w_ids).any(axis=1))[0]
    assert bad.size == 0, (what, "ids differ in rows", bad[:8], ids[bad[:1]], w_ids[bad[:1]])
    live = w_ids >= 0
    assert np.all(np.isneginf(cos[~live])), (what, "padding")
    if live.any():
        assert np.max(np.abs(cos[live] - w_cos[live])) <= 1e-12, (what, "scores")


# ---- seeded inputs, shared by the CPU guard and the GPU tests ---------------------------------------------------------------

def planted(seed, n, d, n_dup=None, noise=0.1):
    """Gaussian rows; n_dup of them overwritten with scaled noisy copies of others (as _planted of the pairs test)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    n_dup = max(1, n // 20) if n_dup is None else n_dup
    if n >= 2:
        src = rng.integers(0, n, n_dup)
        dst = rng.integers(0, n, n_dup)
        x[dst] = x[src] * rng.uniform(0.2, 5.0, (n_dup, 1)).astype(np.float32) + noise * rng.standard_normal((n_dup, d)).astype(np.float32)
    return x


# the exact category's picked combinations: (seed, n, d, top_k, cutoff, noise)
EXACT_CASES = [
    (11, 2, 3, 1, -1.0, 0.1),
    (12, 3, 37, 10, 0.0, 0.1),               # n - 1 < top_k: padding
    (13, 255, 64, 256, -1.0, 0.1),           # n - 1 < top_k on every row
    (14, 256, 257, 10, 0.85, 0.1),
    (15, 257, 768, 64, 0.0, 0.1),
    (16, 1000, 1500, 10, 0.85, 0.2),
    (17, 1000, 3, 1, 0.9999, 0.001),
    (18, 4095, 64, 10, -1.0, 0.1),
    (19, 4096, 37, 64, 0.85, 0.05),
    (20, 4097, 257, 256, 0.0, 0.1),          # the second super-block is one column
    (21, 2500, 4096, 10, 0.85, 0.1),
    (22, 8193, 64, 10, -1.0, 0.1),           # three super-blocks, several growing chunks
    (23, 1000, 768, 256, 0.9999, 0.0005),
]


def fuzz_case(seed):
    """(seed, n, d, top_k, cutoff, noise) of the seeded sweep."""
    rng = np.random.default_rng(77000 + seed)
    n = int(rng.choice([2, 3, 255, 256, 257, 1000, 4095, 4096, 4097]))
    d = int(rng.choice([3, 37, 64, 257, 768, 1500, 4096]))
    top_k = int(rng.choice([1, 10, 64, 256]))
    cutoff = float(rng.choice([-1.0, 0.0, 0.85, 0.9999]))
    if d == 4096:
        n = min(n, 1000)
    noise = float(rng.choice([0.02, 0.1, 0.3])) if cutoff < 0.99 else 0.0005
    return (77000 + seed, n, d, top_k, cutoff, noise)


def exact_input(case):
    seed, n, d, top_k, cutoff, noise = case
    return planted(seed, n, d, noise=noise)


def threshold_input(seed=31, n=8193, d=64, marked=50):
    """`marked` rows whose true nearest neighbour sits in the last 100 rows (the last chunk of every column), and `marked` more
    whose nearest sits in the first 100 (the first chunk).  Returns (x, rows_late, rows_early)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    mid = rng.choice(np.arange(200, n - 200), 2 * marked, replace=False)
    late, early = mid[:marked], mid[marked:]
    tail = rng.choice(np.arange(n - 100, n), marked, replace=False)
    head = rng.choice(np.arange(0, 100), marked, replace=False)
    x[tail] = x[late] * rng.uniform(0.5, 2.0, (marked, 1)).astype(np.float32) + 0.05 * rng.standard_normal((marked, d)).astype(np.float32)
    x[head] = x[early] * rng.uniform(0.5, 2.0, (marked, 1)).astype(np.float32) + 0.05 * rng.standard_normal((marked, d)).astype(np.float32)
    return x, (late, tail), (early, head)


def scaled_copies(seed=5, n=600, d=96):
    """n scaled copies of 3 vectors: every cosine inside a cluster is 1 up to rounding."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((3, d)).astype(np.float32)
    return base[rng.integers(0, 3, n)] * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)


def identical_copies(seed=41, n=1000, d=48, copies=40):
    """`copies` bit-identical rows among n Gaussian ones.  Returns (x, the copies' indices ascending)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    at = np.sort(rng.choice(n, copies, replace=False))
    x[at] = x[at[0]]
    return x, at


# ---- long nomination lists (tests/test_gpu_self_join_lists.py; proven on the CPU in tests/test_knn_ref_host.py) ---------------

def pairs_eps(d_pad):
    """csrc/pairs_common.h: pairs_eps — the bound on |approximate - exact| cosine both self-joins prune with."""
    return 2.0 ** -10 + d_pad * 2.0 ** -23 + 1e-6


def d_pad_of(d):
    """csrc/pairs_common.h: pairs_d_pad."""
    return max(256, (d + 63) // 64 * 64)


LONG_PAIRS_SEED, LONG_PAIRS_N, LONG_PAIRS_THR = 71, 2973, 0.2   # n: the smallest with 256 long columns (the host test counts them)
LONG_PAIRS_OVER = 1024 + 64                        # a column is "long" with more true pairs than one 1024-entry block and a margin


def long_pair_lists(n=LONG_PAIRS_N, seed=LONG_PAIRS_SEED, lead=0):
    """n Gaussian rows in 3 dimensions: about 40 % of all pairs reach cosine 0.2, so column j holds ~0.4 j true pairs and more
    nominees — similar_pairs walks the lists of the last columns in several blocks of 1024.  `lead` zero rows are put in
    FRONT: a zero row pairs with nothing, so the answer is the same pairs shifted by `lead` (Gaussian rows there would add
    ~0.4 (lead n + lead^2 / 2) pairs: 8 million at lead = 4097), while the long columns lie in a later super-block."""
    x = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    return np.concatenate([np.zeros((lead, 3), np.float32), x]) if lead else x


def pairs_from_sim(sim, threshold):
    """(pairs int64 [m][2] ordered by (i, j), cosines float64 [m]): the i < j with sim >= threshold — oracle/cpu_ref.py:
    similar_pairs_f64's loop in one numpy call (its 1.8 M appends take seconds)."""
    i, j = np.nonzero(np.triu(sim >= threshold, 1))
    return np.stack([i, j], axis=1).astype(np.int64), sim[i, j]


TIGHT_SIGMA = 2.5e-3
# (seed, m): one cluster past the finalize's 1024-entry buffer, one past the tighten's 4096 LDS keys
TIGHT_SMALL, TIGHT_LARGE = (101, 1100), (107, 4300)
TIGHT_D, TIGHT_BACKGROUND = 16, 700
# top_k per input: 10 (the reference's), 256 (the limit); 1 on the large input for the probe row
TIGHT_TOP_KS = {TIGHT_SMALL: (10, 256), TIGHT_LARGE: (1, 10, 256)}
TIGHT_PROBE = 0.995                # the large input's probe row (tight_cluster)


def tight_cluster(seed, m, d=TIGHT_D, background=TIGHT_BACKGROUND, sigma=TIGHT_SIGMA, zero_rows=0, group=0, probe=0.0):
    """m rows = one unit vector + sigma x Gaussian noise, each scaled by a factor in [0.2, 5], and `background` Gaussian rows,
    the cluster's indices shuffled through the whole range: a cluster column's nearest neighbours arrive in every chunk of rows
    and in every round of the finalize.  sigma is small enough that every cluster row stays nominated in every cluster column
    (the host test proves it from the oracle), and the noise decides the order: no ties.
    Then, on background rows picked at random: zero_rows of them are zeroed; `group` are overwritten with scaled noisy copies of
    one more (each of the group + 1 has `group` neighbours near cosine 0.99 and hardly another above 0.85); with probe = p one
    becomes a unit row at cosine p to the cluster's centre — for p near 0.99 the whole cluster lies within a few 1e-4 of ITS
    best neighbour, far under its own score of 1: the column whose list is long while its own row must stay out of a_K.
    Returns (x, cluster indices ascending, {"zeroed": indices, "group": indices, "probe": index or -1})."""
    rng = np.random.default_rng(seed)
    centre = rng.standard_normal(d)
    centre /= np.linalg.norm(centre)
    rows = (centre[None, :] + sigma * rng.standard_normal((m, d))) * rng.uniform(0.2, 5.0, (m, 1))
    n = m + background
    perm = rng.permutation(n)
    at, rest = np.sort(perm[:m]), np.sort(perm[m:])
    x = np.empty((n, d), np.float32)
    x[at] = rows.astype(np.float32)
    x[rest] = rng.standard_normal((background, d)).astype(np.float32)
    n_grp = group + 1 if group else 0
    picked = rng.choice(rest, zero_rows + n_grp + 1, replace=False)
    zeroed, grp, at_probe = np.sort(picked[:zero_rows]), np.sort(picked[zero_rows:zero_rows + n_grp]), int(picked[-1])
    x[zeroed] = 0.0
    if group:
        x[grp[1:]] = x[grp[0]] * rng.uniform(0.5, 2.0, (group, 1)).astype(np.float32) + 0.05 * rng.standard_normal((group, d)).astype(np.float32)
    if probe:
        side = rng.standard_normal(d)
        side -= side.dot(centre) * centre
        x[at_probe] = (probe * centre + np.sqrt(1.0 - probe * probe) * side / np.linalg.norm(side)).astype(np.float32)
    return x, at, {"zeroed": zeroed, "group": grp, "probe": at_probe if probe else -1}


def cluster_cosines(sim, at):
    """The float64 cosines of the cluster's pairs i < j."""
    sub = sim[np.ix_(at, at)]
    return sub[np.triu_indices(len(at), 1)]


def tight_cutoffs(sim, at):
    """The cutoffs of the tight-cluster cases: none, the reference's 0.85 (every cluster pair passes, hardly any other)
    and the median in-cluster cosine (half of the cluster's pairs pass: counts differ by row)."""
    return (-1.0, 0.85, float(np.median(cluster_cosines(sim, at))))


def many_identical_copies(seed=109, n=1500, d=8, copies=1300):
    """`copies` bit-identical rows among n Gaussian ones: more than one finalize buffer.  Returns (x, the copies' indices)."""
    return identical_copies(seed, n, d, copies)


def one_dimension(seed=43, n=60):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, 1)).astype(np.float32)
    x[rng.integers(0, n, 3)] = 0.0
    return x


def with_zero_rows(seed=47, n=1000, d=64):
    """Planted rows with n // 50 of them zeroed.  Returns (x, the zeroed indices)."""
    x = planted(seed, n, d, noise=0.1)
    rng = np.random.default_rng(seed + 1)
    z = np.sort(rng.choice(n, n // 50, replace=False))
    x[z] = 0.0
    return x, z
