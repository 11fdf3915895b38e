"""The decoder's layer pieces (csrc/decoder.hip through rarc_lm_rope_table, rarc_lm_rmsnorm, rarc_lm_rowscale_parts, rarc_lm_swiglu,
rarc_lm_attention, rarc_lm_last_logits, rarc_lm_last_embed, rarc_lm_gather_last) in plain float64 numpy, the designed inputs of
tests/test_gpu_decoder_pieces.py and the comparators with their tolerances.  Imported by the tests only.  Every input is the
fp16 array the kernel sees, widened to float64.  None of the tolerances was fitted to a kernel's output.

Rotary table (rope_tolerance).  The reference angle is the float32 product pos * inv_freq with inv_freq = float32(1 /
theta ** (2i / dh)) (oracle.qwen3_last_logits_f32); the reference value is the float64 cos / sin of that angle.  The kernel
computes inv_freq = exp2f(-(2i / dh) * log2f(theta)): 2i / dh is exact; log2f is within one ulp (V_LOG_F32: 1 ulp) of a number in
[8, 32), i.e. 2^-19 absolute; the product with 2i / dh < 1 keeps that and adds half an ulp of a number below 32 (2^-20); an
absolute error e in the exponent is a relative error ln 2 * e in exp2f: ln 2 * 1.5 * 2^-19 = 16.7 fp32 ulps (2^-23); exp2f itself
adds 1; the product pos * inv_freq 0.5; the reference's own inv_freq (powf and a division) is within 1.5 of the exact value.  Sum
19.7: ROPE_K = 20 ulps, so |angle - reference angle| <= pos * inv_freq * 20 * 2^-23, and cos / sin move by at most that.  Pair 0
(inv_freq = exp2f(0) = 1) has no such error.  Added: sincosf (2^-22) and the one fp16 rounding (2^-11 |ref| + 2^-25).

RMSNorm and the endings (rms_bounds, rms_tolerance).  y = half(w * half(x * inv)), inv = 1 / sqrt(mean(x^2) + eps) in fp32.  The
fp32 sum of H positive squares is within H 2^-24 relative, so is inv after division, sqrt and reciprocal with RMS_INV_EPS(H) =
H 2^-24 + 2^-21.  Two comparators, both derived: (1) the analytic one, |got - w x inv| <= |ref| (2^-10 + eps_inv)(1 + 2^-9) +
(|w| + 1) 2^-25 (two fp16 roundings, the subnormal steps); (2) the INTERVAL one, which knows where the roundings fall: with
u = x * inv in float64, half(x * inv) lies between half(u (1 - eps_inv)) and half(u (1 + eps_inv)) — the same number except within
eps_inv of a rounding boundary — and y between the fp16 products of those with w.  (2) rejects a single fp16 ulp anywhere
else; (1) is what is printed.  The logits add an fp32 dot product: 2^-11 |ref| + 2^-25 for the fp16 result, H 2^-24 sum|nv
head| for the accumulation, sum |head| (hi - lo) for the interval of nv.  The embedding without normalisation is nv itself
(interval); normalised: |ref| (out_dim 2^-24 + 2^-21) for the fp32 norm, plus the interval's share.

Row scales from partial sums (rowscale_tolerance): n_parts positive fp32 numbers added, then /H, +eps, sqrt, reciprocal:
|r - ref| <= |ref| (n_parts 2^-24 + 2^-21).

SwiGLU (swiglu_check): against the chain half(half(silu(g)) * u) in float64 within 2 fp16 ulps of max(|want|, 6e-5 max(|u|, 1)) —
the bound tests/test_gpu_reranker_lm.py already sets for the device's __expf (there |u| ~ 1), with its floor — the subnormal step
2^-24 of half(silu(g)) — carried through the product with u like every other error of silu.  Found with the first run: at
g = 2^-24 the fp32 quotient g / (1 + exp(-g)) is exactly the tie 2^-25 (1 + exp(-g) rounds to 2) and rounds to 0, the float64
one lies just above it and rounds to 2^-24; u = 65504 multiplies that one subnormal step.  Infinities must agree.

Attention (attention, attention_tolerance), in two stages because peaked scores are ill-conditioned against the fp16 rounding of
the operands.  Stage (a), qk_operands: the q / k chain with the roundings lm_norm_rope documents (x * inv -> fp16, * w -> fp16,
rotation: the product b * sin -> fp16, then the fused a * cos -+ it -> fp16), cos / sin read from the table passed in (the
device's own).  Stage (b): softmax * V in float64 from those operands over the virtual key index.  Per query and output column:
    tol = sum_j p_j (e^(d_j + D) - 1) |v_j|      d_j = 2^-10 sum_i |q_i k_ij| / sqrt(dh), D = log sum_j p_j e^(d_j)
        + (2^-11 + 2^-18 + n (2^-24 + 2^-25)) max_j |v_j|  +  2^-11 |ref| + 2^-25
  * first line: the kernel's inv is fp32, stage (a)'s float64: an operand element can fall on the other side of a rounding
    boundary, one fp16 ulp (2^-10 relative at most); score j then moves by at most d_j, weight j by e^(d_j) and the normaliser
    by e^D.  (At most e^(2 max d) - 1; weighted by p so that keys that carry no weight do not count.)
  * second line: P is rounded to fp16 in the numerator only (2^-11; the deferred rescale keeps p <= 2^11, same relative
    precision); 2^-18 for the fp32 score (dh products), its scaling and v_exp_f32; n keys are accumulated in fp32 (2^-24 each)
    and a p below 2^-14 of the running maximum is an fp16 subnormal or 0 (2^-25 each); then the one fp16 rounding of the output.
attention_online is the same softmax walked tile by tile like the kernel (running maximum, deferral below 2^11), in float64:
it counts the rescales a case provokes and carries the PLANTED ERRORS of tests/test_lm_ref_host.py."""
import numpy as np

F16_MAX = 65504.0
ROPE_K = 20
DEFER = 11.0
LOG2E = 1.4426950408889634


def f64(a):
    return np.asarray(a).astype(np.float64)


def r16(a):
    """round to fp16 (nearest even, subnormals, overflow to inf) and widen again"""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def h16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def worst(got, ref, tol):
    """max of |got - ref| / tol; anything that is not finite or of another shape counts as infinitely far"""
    got = f64(got)
    if got.shape != np.shape(ref) or not np.isfinite(got).all():
        return np.inf
    return float(np.max(np.abs(got - ref) / tol)) if got.size else 0.0


# --------------------------------------------------------------------------------------------------------------- rotary table
def rope_angles(rows, dh, theta):
    """the reference's float32 angles [rows][dh / 2] and its float32 inv_freq"""
    inv = (1.0 / np.float32(theta) ** (np.arange(0, dh, 2, dtype=np.float32) / np.float32(dh))).astype(np.float32)
    return np.arange(rows, dtype=np.float32)[:, None] * inv[None, :], inv


def rope_table(rows, dh, theta):
    """[rows][dh] float64: cos of the dh / 2 pairs, then their sin"""
    ang = f64(rope_angles(rows, dh, theta)[0])
    return np.concatenate([np.cos(ang), np.sin(ang)], -1)


def rope_tolerance(rows, dh, theta):
    ang, inv = rope_angles(rows, dh, theta)
    k = np.where(np.arange(dh // 2) == 0, 0.0, ROPE_K * 2.0 ** -23)
    dang = np.abs(f64(ang)) * k[None, :] + 2.0 ** -22
    return np.concatenate([dang, dang], -1) + 2.0 ** -11 * np.abs(rope_table(rows, dh, theta)) + 2.0 ** -25


def f16_ulp(x):
    """the fp16 grid step at |x| (2^-24 below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(f64(x)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


# -------------------------------------------------------------------------------------------------------------------- RMSNorm
def rms_inv_eps(H):
    return H * 2.0 ** -24 + 2.0 ** -21


def add_residual(x, delta):
    """half(x + delta): the exact sum rounded once"""
    return r16(f64(x) + f64(delta))


def rms_inv(x, eps):
    x = f64(x)
    return 1.0 / np.sqrt((x * x).mean(-1, keepdims=True) + eps)


def rmsnorm(x, w, eps):
    """w * x * inv in float64, no rounding"""
    return f64(w) * f64(x) * rms_inv(x, eps)


def rmsnorm_chain(x, w, eps):
    """half(w * half(x * inv)) with inv in float64: the documented roundings"""
    return r16(f64(w) * r16(f64(x) * rms_inv(x, eps)))


def rms_tolerance(x, w, eps):
    H = np.shape(x)[-1]
    return np.abs(rmsnorm(x, w, eps)) * (2.0 ** -10 + rms_inv_eps(H)) * (1 + 2.0 ** -9) + (np.abs(f64(w)) + 1) * 2.0 ** -25


def rms_bounds(x, w, eps):
    """(lo, hi): every fp16 value half(w * half(x * inv')) can take for inv' within rms_inv_eps of inv"""
    H = np.shape(x)[-1]
    u, e = f64(x) * rms_inv(x, eps), rms_inv_eps(H)
    t = np.stack([r16(u * (1 - e)), r16(u * (1 + e))])
    y = r16(f64(w) * t)
    return y.min(0), y.max(0)


def within(got, lo, hi):
    got = f64(got)
    return bool(np.isfinite(got).all() and (got >= lo).all() and (got <= hi).all())


def rowscale_parts(ssq, H, eps):
    return 1.0 / np.sqrt(f64(ssq).sum(-1) / H + eps)


def rowscale_tolerance(ssq, H, eps):
    return rowscale_parts(ssq, H, eps) * (np.shape(ssq)[-1] * 2.0 ** -24 + 2.0 ** -21)


RMS_HIDDEN = (8, 128, 512, 520, 640, 1024, 8192)   # one lane; 16 lanes; a full wave; one lane of the second trip; ...; 16 trips
RMS_ROWS = (1, 3, 4, 5, 7)                         # four rows share a workgroup
RMS_INPUTS = ("random", "zero_rows", "full_range", "spike", "subnormal")
RMS_WEIGHTS = ("near_one", "zero_negative_eight")
PARTS_HIDDEN = (128, 1024, 1152, 8192)
PARTS_ROWS = (1, 31, 32, 33)


def rms_input(kind, wkind, rows, H, seed=0):
    """x, delta [rows][H], w [H], all fp16"""
    rng = np.random.default_rng([seed, rows, H, RMS_INPUTS.index(kind), RMS_WEIGHTS.index(wkind)])
    x, delta = rng.standard_normal((rows, H)), rng.standard_normal((rows, H)) * 0.5
    if kind == "zero_rows":                       # x + delta == 0 exactly on the even rows: inv = 1 / sqrt(eps)
        x[::2], delta[::2] = 0, 0
    elif kind == "full_range":                    # rows of +-65504; delta 0 there (the sum must stay an fp16 number)
        x, delta = rng.choice([-F16_MAX, F16_MAX], (rows, H)), np.zeros((rows, H))
    elif kind == "spike":                         # one column of 60000, in another lane and trip for every row
        x, delta = np.zeros((rows, H)), np.zeros((rows, H))
        x[np.arange(rows), (H - 1 + 61 * np.arange(rows)) % H] = 60000
    elif kind == "subnormal":                     # |x| < 2^-14; the sum of squares ~ H 2^-34 is far below eps = 1e-6
        x, delta = rng.integers(-1023, 1024, (rows, H)) * 2.0 ** -24, rng.integers(-8, 9, (rows, H)) * 2.0 ** -24
    w = 1 + rng.uniform(-0.2, 0.2, H)
    if wkind == "zero_negative_eight":
        w = rng.choice([0.0, -1.0, 8.0, -0.37, 1.0], H)
    return h16(x), h16(delta), h16(w)


# --------------------------------------------------------------------------------------------------------------------- SwiGLU
def swiglu_chain(gu, inter):
    """[rows][2 * inter] (groups of 16: 8 gates, their 8 ups) -> half(half(silu(g)) * u) in float64"""
    t = f64(gu).reshape(gu.shape[0], inter // 8, 2, 8)
    g, u = t[:, :, 0].reshape(-1, inter), t[:, :, 1].reshape(-1, inter)
    with np.errstate(over="ignore"):
        return r16(r16(g / (1.0 + np.exp(-g))) * u)


def swiglu_check(got, gu, inter):
    """worst |got - want| in units of the 2-ulp bound; inf if an infinity (or a NaN) disagrees"""
    want, got = swiglu_chain(gu, inter), f64(got)
    u = f64(gu).reshape(gu.shape[0], inter // 8, 2, 8)[:, :, 1].reshape(-1, inter)
    fin = np.isfinite(want)
    if got.shape != want.shape or not np.array_equal(got[~fin], want[~fin]) or not np.isfinite(got[fin]).all():
        return np.inf
    floor = 6e-5 * np.maximum(np.abs(u[fin]), 1.0)
    return float(np.max(np.abs(got[fin] - want[fin]) / (2.0 * np.maximum(np.abs(want[fin]), floor) * 2.0 ** -10)))


def swiglu_input(rows, inter, seed=0):
    rng = np.random.default_rng([seed, rows, inter])
    gates = np.array([F16_MAX, -F16_MAX, 0.0, -0.0, 2.0 ** -24, -2.0 ** -20, 11.0, -11.0, 10.5, -12.0, 1.0, -1.0, 3.0, -4.0, 88.0, -88.0])
    g = rng.standard_normal((rows, inter)) * 3
    u = rng.standard_normal((rows, inter))
    g[:, :16 if inter >= 16 else 8] = gates[:16 if inter >= 16 else 8]
    u[0, ::2], u[0, 1::2] = 0.0, F16_MAX                        # row 0: ups of 0 and 65504 against every special gate
    if rows > 1:
        u[1, ::2], u[1, 1::2] = F16_MAX, 0.0
    t = np.stack([g.reshape(rows, inter // 8, 8), u.reshape(rows, inter // 8, 8)], 2)
    return h16(t.reshape(rows, 2 * inter))


# -------------------------------------------------------------------------------------------------------------------- endings
def last_rows(x, n_seq, row_stride, row_off):
    return f64(x)[np.arange(n_seq) * row_stride + row_off]


def last_logits(x, w, head, eps, n_seq, row_stride, row_off, ids):
    """(ref, tol) [n_seq][2]"""
    xr = last_rows(x, n_seq, row_stride, row_off)
    H = xr.shape[-1]
    nv, (lo, hi) = rmsnorm_chain(xr, w, eps), rms_bounds(xr, w, eps)
    hd = f64(head)[np.asarray(ids)]
    ref = nv @ hd.T
    tol = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + H * 2.0 ** -24 * (np.abs(nv) @ np.abs(hd).T) + (hi - lo) @ np.abs(hd).T
    return ref, tol


def last_embed(x, w, eps, n_seq, row_stride, row_off, out_dim, normalize):
    """(ref, tol) [n_seq][out_dim]; without normalisation tol is the interval's width (0 almost everywhere)"""
    xr = last_rows(x, n_seq, row_stride, row_off)
    nv, (lo, hi) = rmsnorm_chain(xr, w, eps)[:, :out_dim], rms_bounds(xr, w, eps)
    wd = (hi - lo)[:, :out_dim]
    if not normalize:
        return nv, wd
    nr = np.maximum(np.sqrt((nv * nv).sum(-1, keepdims=True)), 1e-12)
    ref = nv / nr
    tol = np.abs(ref) * (out_dim * 2.0 ** -24 + 2.0 ** -21) + wd / nr + np.abs(ref) * np.sqrt((wd * wd).sum(-1, keepdims=True)) / nr
    return ref, tol + 2.0 ** -149


def gather_last(src, L, n_seq, n_rows):
    out = np.zeros((n_rows, src.shape[1]), src.dtype)
    out[:n_seq] = src[np.arange(n_seq) * L + L - 1]
    return out


# ------------------------------------------------------------------------------------------------------------------ attention
def qk_operands(x, w, eps, cs, sn, exact=False, plant=None):
    """x [..][dh] raw rows, cs / sn [..][dh / 2] of each row's position -> RoPE(RMSNorm(x) * w) with the kernel's roundings
    (exact: none).  plant "rotate_sign": rotate_half with the sign flipped."""
    x, w = f64(x), f64(w)
    rnd = (lambda a: a) if exact else r16
    h = x.shape[-1] // 2
    xn = rnd(rnd(x * rms_inv(x, eps)) * w)
    a, b = xn[..., :h], xn[..., h:]
    sg = -1.0 if plant == "rotate_sign" else 1.0
    return np.concatenate([rnd(a * cs - sg * rnd(b * sn)), rnd(b * cs + sg * rnd(a * sn))], -1)


def clamp(v, lo, hi):
    return int(min(max(int(v), lo), hi))


class AttnCase:
    """one call of rarc_lm_attention: fp16 arrays and the geometry"""

    def __init__(self, qkv, start, n_seq, L, n_q, n_kv, dh, q_norm, k_norm, eps=1e-6, cache=None, prefix_of=None, pstart=None,
                 theta=1e6, name=""):
        self.qkv, self.start, self.n_seq, self.L, self.n_q, self.n_kv, self.dh = qkv, np.asarray(start, np.int32), n_seq, L, n_q, n_kv, dh
        self.q_norm, self.k_norm, self.eps, self.cache, self.theta, self.name = q_norm, k_norm, eps, cache, theta, name
        self.prefix_of = None if cache is None else np.asarray(prefix_of, np.int32)
        self.pstart = None if cache is None else np.asarray(pstart, np.int32)
        self.P = 0 if cache is None else cache.shape[1]
        self.n_prefix = 0 if cache is None else cache.shape[0]
        self.rope_rows = self.P + L

    def geometry(self, b, plant=None):
        """(s0, pq, P, u_min, pos_base) of sequence b as the kernels derive them (clamps included)"""
        s0 = clamp(self.start[b], 0, self.L - 1)
        pq = -1 if self.cache is None else int(self.prefix_of[b])
        P = self.P if pq >= 0 else 0
        u_min = clamp(self.pstart[pq], 0, P - 1) if pq >= 0 else 0
        if plant == "start+1":
            s0 = min(s0 + 1, self.L - 1)
        return s0, pq, P, u_min, (0 if pq >= 0 else s0)


def _tables(case, table):
    t = f64(rope_table(case.rope_rows, case.dh, case.theta) if table is None else table)
    return t[:, :case.dh // 2], t[:, case.dh // 2:]


def attention(case, table=None, exact=False, plant=None, online=False):
    """ctx [n_seq * L][n_q * dh] float64 and, unless exact, its tolerance; table: [rope_rows][dh] cos | sin (None: float64 of the
    reference's angles).  With online=True the softmax is walked in 32-key tiles like the kernel (attention_online) and a third
    value reports what the walk did."""
    c, dh, G = case, case.dh, case.n_q // case.n_kv
    cos, sin = _tables(c, table)
    t = f64(c.qkv).reshape(c.n_seq, c.L, c.n_q + 2 * c.n_kv, dh)
    out = np.zeros((c.n_seq, c.L, c.n_q, dh))
    tol = np.zeros_like(out)
    facts = dict(rescales_after_first=0, deferred=0, max_log2_p=-np.inf, tiles=0)
    for b in range(c.n_seq):
        s0, pq, P, u_min, pos_base = c.geometry(b, plant)
        if plant == "umin-1":
            u_min = max(u_min - 1, 0)
        own = np.arange(s0, c.L)
        nk = P + len(own)                                              # virtual keys 0 .. nk - 1 exist
        kpos = np.clip(np.arange(nk) + pos_base, 0, c.rope_rows - 1)
        uq = P + (np.arange(c.L) - s0) + (1 if plant == "causal+1" else 0)   # every row of the sequence is a query
        qpos = np.clip(P + (np.arange(c.L) - s0) + pos_base, 0, c.rope_rows - 1)
        vis = (np.arange(nk)[None, :] >= u_min) & (np.arange(nk)[None, :] <= uq[:, None])
        for kvh in range(c.n_kv):
            src = kvh if plant != "wrong_kv_head" else (kvh + 1) % c.n_kv
            kraw, vraw = t[b, own, c.n_q + src], t[b, own, c.n_q + c.n_kv + src]
            if P:
                pc = f64(c.cache[pq]).reshape(P, 2 * c.n_kv, dh)
                kraw, vraw = np.concatenate([pc[:, src], kraw]), np.concatenate([pc[:, c.n_kv + src], vraw])
            with np.errstate(invalid="ignore", over="ignore"):
                k = qk_operands(kraw, c.k_norm, c.eps, cos[kpos], sin[kpos], exact, plant)
            k, v = np.where(vis.any(0)[:, None], k, 0.0), np.where(vis.any(0)[:, None], vraw, 0.0)   # rows nobody sees: any bits
            for g in range(G):
                hd = kvh * G + g
                with np.errstate(invalid="ignore", over="ignore"):
                    q = qk_operands(t[b, :, hd], c.q_norm if plant != "knorm_for_q" else c.k_norm, c.eps, cos[qpos], sin[qpos], exact, plant)
                q = np.where(vis.any(1)[:, None], q, 0.0)
                s = np.where(vis, q @ k.T / np.sqrt(dh), -np.inf)
                if online:
                    o, f = attention_online(s, v, u_min, plant)
                    for key in ("rescales_after_first", "deferred", "tiles"):
                        facts[key] += f[key]
                    facts["max_log2_p"] = max(facts["max_log2_p"], f["max_log2_p"])
                    out[b, :, hd] = o
                    continue
                m = np.where(vis.any(1), np.max(s, axis=1, initial=-np.inf), 0.0)
                p = np.exp(s - m[:, None])
                den = p.sum(1, keepdims=True)
                p = p / np.where(den > 0, den, 1.0)
                ref = p @ v
                out[b, :, hd] = ref
                if not exact:
                    d = 2.0 ** -10 * (np.abs(q) @ np.abs(k).T) / np.sqrt(dh)
                    D = np.log(np.maximum((p * np.exp(d)).sum(1, keepdims=True), 1.0))
                    vmax = np.max(np.where(vis[:, :, None], np.abs(v)[None], 0.0), axis=1).max(-1, keepdims=True)
                    n = vis.sum(1, keepdims=True)
                    tol[b, :, hd] = ((p * np.expm1(d + D)) @ np.abs(v) + (2.0 ** -11 + 2.0 ** -18 + n * (2.0 ** -24 + 2.0 ** -25)) * vmax
                                     + 2.0 ** -11 * np.abs(ref) + 2.0 ** -25)
    out = out.reshape(c.n_seq * c.L, c.n_q * dh)
    if online:
        return out, facts
    return (out, None) if exact else (out, tol.reshape(out.shape))


def attention_online(s, v, u_min, plant=None):
    """softmax(s) v walked like the kernel: tiles of 32 keys from 32 (u_min / 32), waves of 32 queries, the running maximum
    raised only when some query of the wave exceeds it by more than 2^DEFER (log2 domain), float64 throughout.
    plant "no_rescale": the accumulators keep their scale when the maximum rises after the first tile; "l_not_rescaled": the sum does."""
    nq, nk = s.shape
    t2 = s * LOG2E
    out = np.zeros((nq, v.shape[1]))
    f = dict(rescales_after_first=0, deferred=0, max_log2_p=-np.inf, tiles=0)
    for q0 in range(0, nq, 32):
        sl = slice(q0, min(q0 + 32, nq))
        m = np.full(sl.stop - q0, -np.inf)
        l, o, seen = np.zeros(sl.stop - q0), np.zeros((sl.stop - q0, v.shape[1])), False
        for k0 in range(u_min // 32 * 32, nk, 32):
            tt = t2[sl, k0:k0 + 32]
            if not np.isfinite(tt).any():
                continue
            tmax = tt.max(1)
            f["tiles"] += 1
            if (tmax <= m + DEFER).all():
                f["deferred"] += 1
            else:
                m_new = np.maximum(m, tmax)
                corr = np.where(np.isfinite(m), np.exp2(np.where(np.isfinite(m), m, 0.0) - np.where(np.isfinite(m_new), m_new, 0.0)), 0.0)
                rose = bool((np.isfinite(m) & (m_new > m)).any())
                if rose:
                    f["rescales_after_first"] += 1
                if not (rose and plant == "no_rescale"):
                    o *= corr[:, None]
                if not (rose and plant == "l_not_rescaled"):
                    l *= corr
                m = m_new
            with np.errstate(invalid="ignore"):
                p = np.where(np.isfinite(tt), np.exp2(tt - np.where(np.isfinite(m), m, 0.0)[:, None]), 0.0)
            if p.max() > 0:
                f["max_log2_p"] = max(f["max_log2_p"], float(np.log2(p.max())))
            l += p.sum(1)
            o += p @ v[k0:k0 + 32]
        out[sl] = o / np.where(l > 0, l, 1.0)[:, None]
    return out, f


# --------------------------------------------------------------------------------------------- designed inputs: attention
ATTN_PROFILES = ("flat", "ramp_fast", "ramp_slow", "peak_last", "peak_first", "spike_one")
RAMP_FAST, RAMP_SLOW = 8.0 / 32, 7.4 / 32     # nats per key: 8.0 per tile > 11 ln 2 = 7.62 > 7.4


def boundary_starts(L):
    """0, 1, L - 1 and every multiple of 32 with its two neighbours, as far as they fit"""
    c = {0, 1, L - 1} | {m + d for m in range(32, L + 1, 32) for d in (-1, 0, 1)}
    return sorted(n for n in c if 0 <= n <= L - 1)


def attn_case(profile, dh, n_q, n_kv, L, starts, P=0, pstarts=(), prefix_of=None, seed=0, poison=False, low_rows=None):
    """One designed call.  Every row is a direction in R^dh (RMSNorm forgets its length: rows are scaled by 0.5 .. 2) plus noise;
    the q / k-norm weights carry the gain.  The steering directions live in the two slowest rotary pairs (elements dh/2 - 1 and
    dh/2 - 2: at theta = 1e6 they turn by < 0.02 rad over 8192 positions), so a score is what the profile says to within the
    noise: `ramp_*`: score = c (u - centre) over the virtual key index u; `peak_last`: every query is aligned with its own key
    (score A) and random against the others; `peak_first`: a falling ramp (the first visible key is the maximum, later keys
    fall below 2^-24 of it); `spike_one`: flat, but query 17 of every 32-query block is aligned with the key three rows before
    it; `flat`: random directions, gain ~1.  poison: NaN in every row the contract says is never read; low_rows: value for the
    cache rows in [32 (pstart / 32), pstart) (default: like any other row)."""
    n_seq = len(starts)
    rng = np.random.default_rng([seed, dh, n_q, n_kv, L, P, ATTN_PROFILES.index(profile)])
    U = P + L
    e1, e2 = np.zeros(dh), np.zeros(dh)
    e1[dh // 2 - 1], e2[dh // 2 - 2] = 1, 1
    noise = 0.02 / np.sqrt(dh)
    c = {"ramp_fast": RAMP_FAST, "ramp_slow": RAMP_SLOW, "peak_first": -RAMP_FAST}.get(profile, 0.0)
    A = {"flat": 1.5 * np.sqrt(dh), "peak_last": 24.0, "spike_one": 20.0}.get(profile, abs(c) * U / 2 + 1.0)   # flat: scores ~ N(0, 1.5)
    gq, gk = 1.5 * np.sqrt(A / np.sqrt(dh)), np.sqrt(A / np.sqrt(dh)) / 1.5   # score of aligned unit directions: gq gk sqrt(dh) = A
    q_norm, k_norm = h16(gq * (1 + rng.uniform(-0.05, 0.05, dh))), h16(gk * (1 + rng.uniform(-0.05, 0.05, dh)))
    if profile in ("ramp_fast", "ramp_slow", "peak_first"):   # the steering elements themselves exactly the gain
        for e in (dh // 2 - 1, dh // 2 - 2):
            q_norm[e], k_norm[e] = np.float16(gq), np.float16(gk)

    def kdir(u):                                               # [len(u)][dh]
        if c:
            cosf = np.clip(c * (u - U / 2) / A, -1, 1)
            return cosf[:, None] * e1 + np.sqrt(1 - cosf ** 2)[:, None] * e2
        return None

    def rows(n, base):
        return base + rng.standard_normal((n, dh)) * noise if base is not None else _unit(rng.standard_normal((n, dh)))

    W = n_q + 2 * n_kv
    qkv = np.zeros((n_seq, L, W, dh))
    cache = np.zeros((len(pstarts), P, 2 * n_kv, dh)) if P else None
    for p in range(len(pstarts)):
        for h in range(n_kv):
            cache[p, :, h] = rows(P, kdir(np.arange(P))) * rng.uniform(0.5, 2, (P, 1))
            cache[p, :, n_kv + h] = rng.standard_normal((P, dh))
    for b in range(n_seq):
        s0 = clamp(starts[b], 0, L - 1)
        Pb = P if (P and prefix_of[b] >= 0) else 0
        u = Pb + np.arange(L) - s0
        for h in range(n_kv):
            kd = rows(L, kdir(u))
            qkv[b, :, n_q + h] = kd * rng.uniform(0.5, 2, (L, 1))
            qkv[b, :, n_q + n_kv + h] = rng.standard_normal((L, dh))
            for g in range(n_q // n_kv):
                if c:
                    qd = rows(L, np.broadcast_to(e1, (L, dh)))
                elif profile == "peak_last":
                    qd = _unit(kd) + rng.standard_normal((L, dh)) * noise
                elif profile == "spike_one":
                    qd = rows(L, None) * 0.05 + rng.standard_normal((L, dh)) * noise   # (length is forgotten: still random directions)
                    for i in range(17, L, 32):
                        if i - 3 >= s0:
                            qd[i] = _unit(kd[i - 3])
                else:
                    qd = rows(L, None)
                qkv[b, :, h * (n_q // n_kv) + g] = qd * rng.uniform(0.5, 2, (L, 1))
    qkv = h16(qkv.reshape(n_seq * L, W * dh))
    if cache is not None:
        cache = h16(cache.reshape(len(pstarts), P, 2 * n_kv * dh))
        if low_rows is not None:
            for p, ps in enumerate(pstarts):
                ps = clamp(ps, 0, P - 1)
                cache[p, ps // 32 * 32:ps] = low_rows
    case = AttnCase(qkv, starts, n_seq, L, n_q, n_kv, dh, q_norm, k_norm, cache=cache, prefix_of=prefix_of, pstart=pstarts,
                    name=f"{profile} dh={dh} heads={n_q}/{n_kv} L={L} P={P}")
    return poisoned(case) if poison else case


def _unit(a):
    return a / np.sqrt((a * a).sum(-1, keepdims=True))


def poisoned(case):
    """NaN wherever the contract of rarc_lm_attention says nothing is read: own rows before start (their k | v columns; with no
    prefix the q columns too: the query sees nothing and the select drops the NaN score), cache rows before 32 (pstart / 32)
    and every row of a prefix no sequence names"""
    c = case
    qkv = c.qkv.copy().reshape(c.n_seq, c.L, c.n_q + 2 * c.n_kv, c.dh)
    for b in range(c.n_seq):
        s0, pq, P, u_min, _ = c.geometry(b)
        qkv[b, :s0, (c.n_q if pq >= 0 else 0):] = np.nan
    cache = None
    if c.cache is not None:
        cache = c.cache.copy()
        for p in range(c.n_prefix):
            used = (c.prefix_of == p).any()
            ps = clamp(c.pstart[p], 0, c.P - 1)
            cache[p, :(ps // 32 * 32 if used else c.P)] = np.nan
    return AttnCase(qkv.reshape(c.qkv.shape), c.start, c.n_seq, c.L, c.n_q, c.n_kv, c.dh, c.q_norm, c.k_norm, c.eps, cache, c.prefix_of,
                    c.pstart, c.theta, c.name + " poisoned")


# ------------------------------------------------------------------------------------------------ the pieces chained: a forward
def interleave8(gate, up):
    """RarcLmLayer.gate_up_w: 8 gate_proj rows, then the 8 up_proj rows of the same features"""
    i, h = gate.shape
    return np.stack([gate.reshape(i // 8, 8, h), up.reshape(i // 8, 8, h)], 1).reshape(2 * i, h)


def forward_logits(sd, cfg, ids, start, token_ids, exact=True, row_off=None):
    """The references above chained into the whole forward (left padded: start[b] = first real token), float64.  exact: no fp16
    emulation anywhere — the function of oracle.qwen3_last_logits_f32.  row_off: the row the final norm reads (default L - 1)."""
    g = lambda k: f64(sd[k])
    ids = np.asarray(ids)
    n, L = ids.shape
    nq, nkv, dh = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps, theta = float(cfg.get("rms_norm_eps", 1e-6)), float(cfg.get("rope_theta", 1e6))
    rnd = (lambda a: a) if exact else r16
    x = g("model.embed_tokens.weight")[ids].reshape(n * L, -1)
    i = 0
    while f"model.layers.{i}.self_attn.q_proj.weight" in sd:
        p = f"model.layers.{i}."
        h = rnd(rmsnorm(x, g(p + "input_layernorm.weight"), eps)) if exact else rmsnorm_chain(x, g(p + "input_layernorm.weight"), eps)
        wqkv = np.concatenate([g(p + f"self_attn.{nme}_proj.weight") for nme in ("q", "k", "v")])
        case = AttnCase(rnd(h @ wqkv.T), start, n, L, nq, nkv, dh, g(p + "self_attn.q_norm.weight"), g(p + "self_attn.k_norm.weight"), eps,
                        theta=theta)
        ctx = rnd(attention(case, exact=exact)[0])
        x = rnd(x + rnd(ctx @ g(p + "self_attn.o_proj.weight").T))
        w = g(p + "post_attention_layernorm.weight")
        h = rmsnorm(x, w, eps) if exact else rmsnorm_chain(x, w, eps)
        gate, up = rnd(h @ g(p + "mlp.gate_proj.weight").T), rnd(h @ g(p + "mlp.up_proj.weight").T)
        act = rnd(rnd(gate / (1.0 + np.exp(-gate))) * up)
        x = rnd(x + rnd(act @ g(p + "mlp.down_proj.weight").T))
        i += 1
    xr = last_rows(x, n, L, L - 1 if row_off is None else row_off)
    w = g("model.norm.weight")
    nv = rmsnorm(xr, w, eps) if exact else rmsnorm_chain(xr, w, eps)
    head = g("lm_head.weight") if "lm_head.weight" in sd else g("model.embed_tokens.weight")
    return nv @ head[np.asarray(token_ids)].T


# ----------------------------------------------------------------------------------------- the designed calls of the GPU test
ATTN_L = (1, 31, 32, 33, 63, 64, 65, 96, 160)
GROUPS = {1: (2, 2), 2: (4, 2), 3: (3, 1), 4: (4, 1)}          # G = n_q / n_kv -> (n_q, n_kv)
# per head_dim: the smallest and the largest length of every resident instantiation NP = 2 .. 5 not met in ATTN_L (keys = the
# length rounded up to 32; NP = ceil(keys / 64) at head_dim 128, ceil(keys / 128) at 64), then one length past the last
RESIDENT_L = {128: (128, 192, 224, 256, 288), 64: (256, 288, 384, 416, 512, 544)}
PAST_RESIDENT_L = {128: 320, 64: 545}
PREFIX_P = (32, 64, 96)


def _chunks(v, n):
    return [v[i:i + n] for i in range(0, len(v), n)]


def attn_cases():
    """[(id, kwargs of attn_case)]: every call tests/test_gpu_decoder_pieces.py makes (and tests/test_lm_ref_host.py plants errors in)"""
    out, i = [], 0
    for dh in (64, 128):
        for L in ATTN_L:                                        # a. every length x every boundary start, profiles and G cycling
            for st in _chunks(boundary_starts(L), 4):
                n_q, n_kv = GROUPS[1 + i % 4]
                out.append(dict(profile=ATTN_PROFILES[i % 6] if L >= 33 else "flat", dh=dh, n_q=n_q, n_kv=n_kv, L=L, starts=st))
                i += 1
        for L in (96, 160):                                     # b. every score profile over three and five tiles
            for prof in ATTN_PROFILES:
                out.append(dict(profile=prof, dh=dh, n_q=4, n_kv=2, L=L, starts=[0, 1, 33, L - 1]))
        for j, L in enumerate(RESIDENT_L[dh] + (PAST_RESIDENT_L[dh],)):   # c. the resident instantiations and one length past them
            out.append(dict(profile=("flat", "peak_last", "spike_one")[j % 3], dh=dh, n_q=2, n_kv=1, L=L, starts=[0, 37]))
        for P, L in ((96, 192), (32, 256)) if dh == 128 else ((64, 480), (96, 448)):   # the largest class with a prefix in it
            out.append(dict(profile="peak_last", dh=dh, n_q=2, n_kv=1, L=L, starts=[0, 37], P=P, pstarts=[5, 0], prefix_of=[0, -1]))
        for P in PREFIX_P:                                      # d. prefixes: every pstart, owners mixed with -1, one prefix unused
            ps = sorted({p for p in (0, 1, 31, 32, 33, P - 1) if p <= P - 1})
            for k, grp in enumerate(_chunks(list(range(len(ps))), 3)):
                prof = ("ramp_fast", "peak_first", "flat", "ramp_slow")[i % 4]
                owners = ([-1] + grp + grp)[:4]
                L = (40, 65)[k % 2]
                out.append(dict(profile=prof, dh=dh, n_q=4, n_kv=2, L=L, starts=[0, 5, 33, L - 1][:len(owners)], P=P, pstarts=ps + [7],
                                prefix_of=owners))
                i += 1
        # e. start and pstart outside their ranges: the kernels clamp them, the reference with them
        out.append(dict(profile="peak_first", dh=dh, n_q=2, n_kv=2, L=65, starts=[-5, 68, 65, -1]))
        out.append(dict(profile="peak_first", dh=dh, n_q=2, n_kv=2, L=40, starts=[-5, 43, 3, 0], P=32, pstarts=[-2, 37, 32, 3],
                        prefix_of=[0, 1, 2, -1]))
    return [(f"{n:03d}-{kw['profile']}-dh{kw['dh']}-g{kw['n_q'] // kw['n_kv']}-L{kw['L']}-P{kw.get('P', 0)}", kw) for n, kw in enumerate(out)]
