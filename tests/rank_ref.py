"""Plain restatements of the rank-level operations (csrc/fuse.hip, the merge in csrc/finalize.hip) that share no code with the
kernels or with the host mirrors, plus the seeded input generators the host and the GPU tests both use.

  rrf          oracle.rrf_fuse is the definition (a dict and python floats); rrf_rows() only shapes it like fuse_ids' outputs.
  rerank       oracle.stable_desc_order of the scores the kernel itself produced, and is_permutation().
  merge        sorted() with an explicit comparator over (score, id) pairs: score descending, +0.0 above -0.0, id ascending.
  mmr          MMRRef: the greedy loop with dots and norms in np.longdouble (64-bit significand) over EXACT products; at each step
               the best value and the set of candidates within `tol` of it.  mmr_tol() is the derived bound on how far the
               kernel's sequential fp64 evaluation can stray.

tests/test_rank_ref_host.py holds these to what the repository already pins, before a GPU is involved.
"""
import functools
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than float64 here: the MMR reference needs the x87 format"
U = 2.0 ** -53          # unit roundoff of fp64


# ------------------------------------------------------------------------------------------------------------------ rerank
def is_permutation(perm, n: int) -> bool:
    p = np.asarray(perm).astype(np.int64).ravel()
    return p.size == n and bool(np.array_equal(np.sort(p), np.arange(n)))


def rerank_order(oracle, scores_row):
    """The order the reranker owes for one row of ITS scores: stable, descending, NaN last in input order."""
    order = oracle.stable_desc_order(scores_row)
    assert is_permutation(order, len(scores_row))
    return order


def p_yes_f64(z_no, z_yes):
    """exp(log_softmax([no, yes])[1]) with the arithmetic in float64 and the reference's two fp16 tensors (the log-softmax
    output, the exp output) where the reference has them.  Returns float16."""
    zn, zy = np.asarray(z_no, np.float16).astype(np.float64), np.asarray(z_yes, np.float16).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.maximum(zn, zy)
        ls = ((zy - m) - np.log(np.exp(zn - m) + np.exp(zy - m))).astype(np.float16)
        return np.exp(ls.astype(np.float64)).astype(np.float16)


RERANK_NS = (1, 2, 255, 256, 257, 1000, 4096)
RERANK_FINITE_ROWS = 6


def rerank_rows(n):
    """(z_no, z_yes fp16 [9][n], finite bool [9]) for one n.  Finite rows (every p_yes a number): ordinary logits; long runs
    of exact ties; an all-equal row; logits at +-65504; -inf against a finite logit; ties between the saturated ends.  The
    other rows mix (inf, inf), (-inf, -inf), NaN and one-sided +inf pairs into ordinary ones: their p_yes is NaN."""
    rng = np.random.default_rng([n, 31])
    zn = (rng.standard_normal((9, n)) * 4).astype(np.float16)
    zy = (rng.standard_normal((9, n)) * 4).astype(np.float16)
    run = rng.integers(0, 5, n)                                      # row 1: five distinct pairs only
    zn[1], zy[1] = zn[1, run], zy[1, run]
    zn[2], zy[2] = zn[2, 0], zy[2, 0]                                # row 2: all equal
    big = rng.random(n) < 0.5                                        # row 3: the largest finite fp16 values, either sign
    zn[3, big] = np.where(rng.random(int(big.sum())) < 0.5, 65504, -65504)
    zy[3, big] = np.where(rng.random(int(big.sum())) < 0.5, 65504, -65504)
    pick = rng.integers(0, 3, n)                                     # row 4: -inf against a finite logit, either side
    zn[4, pick == 1] = -np.inf
    zy[4, pick == 2] = -np.inf
    zn[5], zy[5] = np.where(run < 2, -65504, zn[5]), np.where(run < 2, 65504, zy[5])   # row 5: many p_yes = 1 exactly,
    zy[5, run == 4], zn[5, run == 4] = -np.inf, 0                                      # and many 0 exactly
    kind = rng.integers(0, 8, (3, n))                                # rows 6..8: NaN p_yes among ordinary ones
    for r in range(3):
        k_ = kind[r]
        zn[6 + r, k_ == 0], zy[6 + r, k_ == 0] = np.inf, np.inf
        zn[6 + r, k_ == 1], zy[6 + r, k_ == 1] = -np.inf, -np.inf
        zn[6 + r, k_ == 2] = np.nan
        zy[6 + r, k_ == 3] = np.nan
        zn[6 + r, k_ == 4] = np.inf                                  # inf - inf inside the max subtraction
    zn[8, : n // 2], zy[8, : n // 2] = np.inf, np.inf                # a long run of NaN at the FRONT of the row
    finite = np.arange(9) < RERANK_FINITE_ROWS
    return zn, zy, finite


# --------------------------------------------------------------------------------------------------------------------- rrf
def rrf_rows(oracle, keys, lens, rrf_k, top_k):
    """[(fused keys, fp64 scores)] per query of keys int64 [nq][n_lists][max_len], lens [nq][n_lists]."""
    out = []
    for b in range(keys.shape[0]):
        want = oracle.rrf_fuse([keys[b, r, : lens[b, r]].tolist() for r in range(keys.shape[1])], rrf_k, top_k)
        out.append(([k for k, _ in want], [s for _, s in want]))
    return out


RRF_POPULATIONS = ("distinct", "everywhere", "hot", "tiny", "wide")


def rrf_keys(rng, nq, n_lists, max_len, population):
    """int64 [nq][n_lists][max_len] keys of one population (see RRF_POPULATIONS)."""
    total = n_lists * max_len
    keys = np.empty((nq, n_lists, max_len), np.int64)
    for b in range(nq):
        if population == "distinct":
            flat = rng.permutation(total).astype(np.int64) + 1
        elif population == "everywhere":           # one key in EVERY list (at a different position in each), the rest distinct
            flat = (rng.permutation(total).astype(np.int64) + 1).reshape(n_lists, max_len)
            if max_len:
                flat[np.arange(n_lists), rng.integers(0, max_len, n_lists)] = 777_777_777
            flat = flat.ravel()
        elif population == "hot":                  # a few hot keys, repeated inside one list too
            flat = rng.permutation(total).astype(np.int64) + 1
            hot = rng.random(total) < 0.2
            flat[hot] = rng.integers(-3, 0, int(hot.sum()))
        elif population == "tiny":                 # an alphabet of 7 keys: occurrence chains hundreds of links long
            flat = rng.integers(0, 7, total).astype(np.int64)
        elif population == "wide":                 # 0 (what dead lanes compare against), negatives, >= 2^32, the extremes
            pool = np.array([0, -1, -2, 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 5, -(2 ** 35), 2 ** 63 - 1, -(2 ** 63)], np.int64)
            flat = np.where(rng.random(total) < 0.3, pool[rng.integers(0, pool.size, total)],
                            rng.integers(-(2 ** 62), 2 ** 62, total)).astype(np.int64)
        else:
            raise ValueError(population)
        keys[b] = flat.reshape(n_lists, max_len)
    return keys


def rrf_lens(rng, nq, n_lists, max_len, total, ragged):
    """int32 [nq][n_lists] lengths summing to `total` in query 0 (and 2, 4, ...); odd queries get other totals, so adjacent
    blocks differ.  ragged: lengths vary per list and include 0."""
    lens = np.zeros((nq, n_lists), np.int32)
    for b in range(nq):
        want = total if b % 2 == 0 else int(rng.integers(0, total + 1))
        if not ragged:
            full, rest = divmod(want, max_len) if max_len else (0, 0)
            lens[b, :full] = max_len
            if full < n_lists:
                lens[b, full] = rest
            continue
        left = want
        order = rng.permutation(n_lists)
        for j, r in enumerate(order):
            room = (n_lists - 1 - j) * max_len              # what the lists after this one can still hold
            lo = max(0, left - room)
            hi = min(max_len, left)
            take = hi if j == n_lists - 1 else int(rng.integers(lo, hi + 1))
            if j % 5 == 0 and lo == 0:
                take = 0
            lens[b, r] = take
            left -= take
        assert left == 0 or lens[b].sum() <= want
    return lens


# ------------------------------------------------------------------------------------------------------------------- merge
def _better(a, b):
    """cmp for (score, id) pairs: negative when a ranks ahead of b.  Score descending; of two zeros +0.0 ranks ahead of -0.0
    (the order of a single-shard search, whose keys are the sign-magnitude bit patterns); then id ascending."""
    sa, sb = a[0], b[0]
    if sa > sb:
        return -1
    if sa < sb:
        return 1
    if sa == 0.0 and sb == 0.0:
        na, nb = math.copysign(1.0, sa) < 0, math.copysign(1.0, sb) < 0
        if na != nb:
            return 1 if na else -1
    return -1 if a[1] < b[1] else (1 if a[1] > b[1] else 0)


def merge(ids, scores, k):
    """[G][nq][kk] per-shard answers -> ([nq][k] ids, [nq][k] fp32 scores); entries with id < 0 do not exist; the tail of a
    query with fewer than k entries is (-1, -inf).  NaN scores are outside this restatement."""
    G, nq, kk = ids.shape
    out_i = np.full((nq, k), -1, np.int64)
    out_s = np.full((nq, k), -np.inf, np.float32)
    for q in range(nq):
        pairs = [(float(scores[g, q, j]), int(ids[g, q, j])) for g in range(G) for j in range(kk) if ids[g, q, j] >= 0]
        pairs = sorted(pairs, key=functools.cmp_to_key(_better))[:k]
        for i, (s, d) in enumerate(pairs):
            out_i[q, i], out_s[q, i] = d, np.float32(s)
    return out_i, out_s


def merge_inputs(rng, G, nq, k):
    """Shard answers as shards give them (each list sorted by the order above), built to hurt: ids over [0, 2^63); scores from
    a small set so that most comparisons are decided by id; query 0 all-empty; query 1 fewer than k valid entries in total;
    short shards elsewhere; signed zeros."""
    ids = rng.integers(0, 2 ** 63, (G, nq, k), dtype=np.int64)
    levels = np.array([-np.inf, -3.5, -1.0, -0.0, 0.0, 2.0 ** -140, 0.25, 0.25000003, 7.0, 3.0e38], np.float32)
    sc = np.where(rng.random((G, nq, k)) < 0.7, levels[rng.integers(0, levels.size, (G, nq, k))],
                  rng.standard_normal((G, nq, k))).astype(np.float32)
    n_valid = rng.integers(0, k + 1, (G, nq))
    n_valid[rng.random((G, nq)) < 0.5] = k
    if nq > 0:
        n_valid[:, 0] = 0
    if nq > 1:
        n_valid[:, 1] = 0
        n_valid[G - 1, 1] = max(1, k // 3) if G * k > 1 else 0
    if nq > 2:
        n_valid[:, 2] = k
        sc[:, 2, :] = 0.25                       # everything ties: id ascending across all shards
    for g in range(G):
        for q in range(nq):
            nv = int(n_valid[g, q])
            pairs = sorted(((float(sc[g, q, j]), int(ids[g, q, j])) for j in range(nv)), key=functools.cmp_to_key(_better))
            for j, (s, d) in enumerate(pairs):
                sc[g, q, j], ids[g, q, j] = s, d
            sc[g, q, nv:], ids[g, q, nv:] = -np.inf, -1
    return ids, sc


# --------------------------------------------------------------------------------------------------------------------- mmr
def exact_dots(A, B):
    """A @ B.T as np.longdouble, every product exact.  Inputs on a binary grid coarse enough that a float64 dot cannot round
    (the generated cases) go through one float64 matmul; anything else through Fractions (small recorded cases)."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    d = A.shape[1]
    for g in (7, 10, 16, 20):
        sa, sb = A * 2.0 ** g, B * 2.0 ** g
        if np.array_equal(sa, np.rint(sa)) and np.array_equal(sb, np.rint(sb)):
            if d * max(np.abs(sa).max(initial=0.0), 1.0) * max(np.abs(sb).max(initial=0.0), 1.0) < 2.0 ** 53:
                return (A @ B.T).astype(LD)            # integers below 2^53 scaled by a power of two: exact in any order
            break
    out = np.empty((A.shape[0], B.shape[0]), LD)
    fa = [[Fraction(float(v)) for v in row] for row in A]
    fb = [[Fraction(float(v)) for v in row] for row in B]
    for i, ra in enumerate(fa):
        for j, rb in enumerate(fb):
            s = sum((x * y for x, y in zip(ra, rb)), Fraction(0))
            hi = float(s)
            out[i, j] = LD(hi) + LD(float(s - Fraction(hi)))
    return out


def mmr_tol(d, nu_q, nu_c, normalize, lam):
    """Twice the bound on |value the kernel computes - true value| for one candidate, so that the kernel's pick, whose
    COMPUTED value is the largest, has a TRUE value within mmr_tol of the true best.  u = 2^-53.

    normalize = 0.  A d-term sequential fp64 dot of vectors of norm at most nu has error <= d u nu_a nu_b, so
        E = d u max(nu_q nu_c, nu_c^2)                   for <q, e_i> and for every <e_s, e_i> (hence for their running maximum).
    normalize = 1.  sum of squares: relative error <= d u; its root: <= (d / 2 + 1) u; each element v / nr: <= (d / 2 + 2) u;
        a product of two such elements: <= (d + 5) u; the d-term sum over unit vectors: <= d u more.  E = (2 d + 8) u, nu = 1.
    value = lam qsim - (1 - lam) mx: the errors enter as lam E + (1 - lam) E = E; rounding (1 - lam), the two products and the
    difference adds at most 4 u (lam |qsim| + (1 - lam) |mx|) <= 4 u M with M = max(nu_q nu_c, nu_c^2).
    lam does not appear: the bound holds for every lam in [0, 1]."""
    assert 0.0 <= lam <= 1.0
    M = 1.0 if normalize else max(nu_q * nu_c, nu_c * nu_c)
    E = (2 * d + 8) * U if normalize else d * U * M
    return 2.0 * (E + 4.0 * U * M)


class MMRRef:
    """State of the greedy selection of _mmr_select (pick 0 first; then value_i = lam <q, e_i> - (1 - lam) max(0, max over
    the selected s of <e_s, e_i>), the first largest) in np.longdouble.  The caller walks: step() describes the choice on
    offer, take(i) commits ANY candidate — so a kernel's own picks can be followed and judged one at a time."""

    def __init__(self, cand, query, normalize, lam):
        E = np.asarray(cand, np.float32).astype(np.float64)            # the kernel's candidates are fp32
        q = np.asarray(query, np.float64)
        self.n, self.d = E.shape
        gram = exact_dots(E, E)
        qs = exact_dots(E, q[None, :])[:, 0]
        self.nu_c = float(np.sqrt(np.max(np.diag(gram))))
        self.nu_q = float(np.sqrt(exact_dots(q[None, :], q[None, :])[0, 0]))
        if normalize:
            cn, qn = np.sqrt(np.diag(gram)), np.sqrt(exact_dots(q[None, :], q[None, :])[0, 0])
            gram = gram / (cn[:, None] * cn[None, :])
            qs = qs / (cn * qn)
        self.gram, self.qsim = gram, qs
        self.lam, self.one_minus = LD(lam), LD(1.0) - LD(lam)          # both exact in 64 bits
        self.tol = mmr_tol(self.d, self.nu_q, self.nu_c, normalize, lam)
        self.taken = np.zeros(self.n, bool)
        self.maxsim = np.zeros(self.n, LD)
        self.take(0)

    def take(self, i):
        assert 0 <= i < self.n and not self.taken[i]
        self.taken[i] = True
        self.maxsim = np.maximum(self.maxsim, self.gram[i])

    def step(self):
        """(best value, indices within tol of it ascending, all values with the selected ones at -inf)."""
        val = self.lam * self.qsim - self.one_minus * self.maxsim
        val = np.where(self.taken, LD(-np.inf), val)
        best = val.max()
        return best, np.flatnonzero(val >= best - LD(self.tol)), val


def mmr_inputs(n, d, seed, ties):
    """(cand fp32 [n][d], query fp64 [d]) on the grid of 1/128: clustered vectors sharing a positive offset, so that every
    pairwise similarity is positive and the redundancy term is never clamped at 0.  ties=True adds a copy of the query and exact
    duplicates (of candidate 0, of each other, of the query copy)."""
    rng = np.random.default_rng([n, d, seed])
    n_c = max(1, n // 8)
    centres = rng.integers(-256, 257, (n_c, d))
    E = centres[rng.integers(0, n_c, n)] + rng.integers(-24, 25, (n, d)) + 300
    q = centres[rng.integers(0, n_c)] + rng.integers(-24, 25, d) + 300
    if ties and n > 3:
        E[n // 2] = q                                       # (once picked, every i with max sim = <q, e_i> has lam-0.5 value 0)
    if ties and n > 1:
        for a, b in ((0, 1), (2, n - 1), (n // 2, n // 3), (5, 7), (7, 11), (n // 4, n // 4 + 1)):
            if a < n and b < n and a != b and n > 3:
                E[b] = E[a]
        if n <= 3:
            E[n - 1] = E[0]
    return (E / 128.0).astype(np.float32), (q / 128.0).astype(np.float64)


MMR_NS = (1, 2, 255, 256, 257, 600, 1024)
MMR_DS = (1, 3, 64, 384, 768)
MMR_LAMBDAS = (0.0, 0.3, 0.5, 1.0)


def mmr_cases(n, d):
    """The (lam, normalize, ties, seed) variants run for one (n, d): every lam x normalize without built ties, and every
    lam x normalize with them."""
    return [(lam, nm, ties, 17 + 2 * j + nm) for ties in (False, True) for j, lam in enumerate(MMR_LAMBDAS) for nm in (0, 1)]


def mmr_ties_built(n, d, ties):
    """Cases that contain exact ties by construction: the duplicated ones, and d = 1 (one axis: few distinct directions)."""
    return ties or d == 1


def mmr_check_walk(ref, picks, what):
    """Follow `picks` (the kernel's, or anyone's) through ref.  Each pick after the first must lie in the near-best set, must
    BE it when that set has one member, and must be the lowest index among the near-best candidates whose value is exactly
    the pick's (identical rows, identical history: identical arithmetic in any implementation).  Returns the number of steps
    whose near-best set had more than one member."""
    assert picks[0] == 0, f"{what}: first pick {picks[0]}"
    wide = 0
    for step, p in enumerate(picks[1:], 1):
        best, near, val = ref.step()
        assert p in near, f"{what}: step {step} picked {p} (value {val[p] if 0 <= p < ref.n else '?'}) but the best is {best} at {near[:8]}"
        if near.size == 1:
            assert p == near[0]
        else:
            wide += 1
            same = [i for i in near if np.array_equal(ref.gram[i], ref.gram[p]) and ref.qsim[i] == ref.qsim[p]]
            assert p == min(same), f"{what}: step {step} picked {p}, not the lowest of the exactly equal {same[:8]}"
        ref.take(int(p))
    return wide
