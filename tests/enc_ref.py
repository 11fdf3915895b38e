"""The encoder's layer pieces (csrc/encoder.hip: rarc_enc_embed_ln, rarc_enc_add_ln, rarc_enc_attention, rarc_enc_pool,
rarc_enc_pool_mean) in plain float64 numpy, the designed inputs of tests/test_gpu_encoder_pieces.py and the comparators with
their tolerances.  Imported by the tests only.  Every input is the fp16 array the kernel sees, widened to float64.

Tolerances (derived from the kernels' arithmetic and the number formats; none was fitted to a kernel's output)

LayerNorm pieces (ln_tolerance).  The kernel reads fp16, works in fp32 and rounds once to fp16:
    |got - ref| <= 2^-11 |ref| + 2^-25 + C 2^-24 |gamma_j| (max|x_row| + |mean|) / sqrt(var + eps)
  * 2^-11 |ref| + 2^-25 is the one fp16 rounding (half an ulp of an 11-bit significand; half the subnormal step 2^-24).
  * the last term is the fp32 arithmetic in front of it.  Every fp32 operation adds at most 2^-24 of its result, the results
    are bounded by max|x_row| + |mean|, and an error e in (x - mean) reaches the output as e |gamma_j| / sqrt(var + eps).
    Operations on the path of one output of ln_row: the row sum (16 in-lane adds, 6 butterfly levels) and its division by H = 23;
    the sum of squares (per element a subtract and an fma, 16 of them in a lane, 6 levels), its division, the add of eps and the
    rsqrt: counted per result that feeds the next one = 16 + 6 + 3 = 25; the output's subtract, two multiplies and the add of
    beta = 4; the adds that form x (one for x + resid, two for word + pos + type) = 2.  54 in all: C = 64, the next power of two.
  On ordinary rows (|x| ~ 1, var ~ 1) that term is 64 * 6e-8 * 4 ~ 1.5e-5, far below half an fp16 ulp of an output of size 1
  (4.9e-4): it exists for rows with a large mean and a small variance, where the cancellation in x - mean multiplies it.

Attention (attention_tolerance).  The output is a convex combination of the V rows of the real keys, so every error term is
relative to max|V| over the real keys of that (sequence, head): P is rounded to fp16 in the numerator only (2^-11), __expf is
about 2^-14 relative for |x| <= 88, the output takes one fp16 rounding (2^-11).  Their sum is 2^-10 + 2^-14; allowed is
    |got - ref| <= 2^-9 max|V|      (about twice that sum: the fp32 accumulation and the score's own rounding are the rest)

Pools (pool_mean_tolerance).  CLS pooling without normalisation is exact (out == float32(hidden[b * L]), compared on the bits).
Mean pooling adds len tokens one after the other in fp32 and divides once: len - 1 roundings of partial sums that are at most
sum|x| and one of the quotient, so per column
    |got - ref| <= len 2^-24 sum_t |x_t|
With normalisation both pools claim the canonical order of prep.hip: checked on the bits against rarc_l2norm_rows_f32 of the
un-normalised output, not with a tolerance."""
import numpy as np

LN_C = 64
F16_MAX = 65504.0


def f64(a):
    return np.asarray(a).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------- references
def layer_norm(z, gamma, beta, eps):
    z = f64(z)
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).mean(-1, keepdims=True)
    return (z - mean) / np.sqrt(var + eps) * f64(gamma) + f64(beta)


def embed_sum(ids, word, pos, type0, seq_len):
    """word[ids[t]] + pos[t % seq_len] + type0, ids clamped into the table as the kernel clamps them"""
    word = f64(word)
    ids = np.clip(np.asarray(ids, np.int64).reshape(-1), 0, word.shape[0] - 1)
    return word[ids] + f64(pos)[np.arange(ids.size) % seq_len] + f64(type0)


def embed_ln(ids, word, pos, type0, gamma, beta, eps, seq_len):
    return layer_norm(embed_sum(ids, word, pos, type0, seq_len), gamma, beta, eps)


def add_ln(x, resid, gamma, beta, eps):
    return layer_norm(f64(x) + f64(resid), gamma, beta, eps)


def clamp_lens(lens, L):
    return np.clip(np.asarray(lens, np.int64), 1, L)


def split_qkv(qkv, n_seq, L, heads, dh):
    """q, k, v as [n_seq][heads][L][dh] from the fused [n_seq * L][3 * heads * dh] matrix (q | k | v, heads contiguous in each)"""
    t = f64(qkv).reshape(n_seq, L, 3, heads, dh)
    return tuple(t[:, :, i].transpose(0, 2, 1, 3) for i in range(3))


def attention(qkv, lens, n_seq, L, heads, dh):
    """softmax(Q K^T / sqrt(dh)) V over the keys < lens[b]; a list of [lens[b]][heads * dh] arrays: real query rows only"""
    q, k, v = split_qkv(qkv, n_seq, L, heads, dh)
    out = []
    for b, n in enumerate(clamp_lens(lens, L)):
        s = q[b, :, :n] @ k[b, :, :n].transpose(0, 2, 1) / np.sqrt(dh)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        out.append((p @ v[b, :, :n]).transpose(1, 0, 2).reshape(n, heads * dh))
    return out


def l2_normalize(x):
    nr = np.sqrt((x * x).sum(-1, keepdims=True))
    return np.where(nr > 0, x / np.where(nr > 0, nr, 1.0), x)


def pool_cls(hidden, L, normalize):
    h = f64(hidden)
    out = h.reshape(-1, L, h.shape[-1])[:, 0]
    return l2_normalize(out) if normalize else out


def pool_mean(hidden, lens, L, normalize):
    h = f64(hidden)
    h = h.reshape(-1, L, h.shape[-1])
    out = np.stack([h[b, :n].sum(0) / n for b, n in enumerate(clamp_lens(lens, L))])
    return l2_normalize(out) if normalize else out


# -------------------------------------------------------------------------------------------------------------- comparators
def ln_tolerance(z, gamma, eps, ref):
    """z: the float64 row sums that enter the LayerNorm ([rows][H]); ref = layer_norm(z, ...)"""
    z = f64(z)
    mean = z.mean(-1, keepdims=True)
    var = ((z - mean) ** 2).mean(-1, keepdims=True)
    fp32 = LN_C * 2.0 ** -24 * np.abs(f64(gamma)) * (np.abs(z).max(-1, keepdims=True) + np.abs(mean)) / np.sqrt(var + eps)
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + fp32


def worst(got, ref, tol):
    """max of |got - ref| / tol; anything that is not finite counts as infinitely far"""
    got = f64(got)
    if got.shape != np.shape(ref) or not np.isfinite(got).all():
        return np.inf
    return float(np.max(np.abs(got - ref) / tol)) if got.size else 0.0


def ln_worst(got, z, gamma, beta, eps):
    ref = layer_norm(z, gamma, beta, eps)
    return worst(got, ref, ln_tolerance(z, gamma, eps, ref))


def attention_tolerance(qkv, lens, n_seq, L, heads, dh):
    """[n_seq][heads]: 2^-9 max|V| over the real keys"""
    v = split_qkv(qkv, n_seq, L, heads, dh)[2]
    return np.stack([2.0 ** -9 * np.abs(v[b, :, :n]).max(axis=(1, 2)) for b, n in enumerate(clamp_lens(lens, L))])


def attention_worst(got, ref, qkv, lens, n_seq, L, heads, dh):
    """got: [n_seq * L][heads * dh] as the kernel writes it (or a list like `ref`); only the real query rows are compared"""
    tol = attention_tolerance(qkv, lens, n_seq, L, heads, dh)
    w = 0.0
    for b, n in enumerate(clamp_lens(lens, L)):
        g = got[b] if isinstance(got, list) else f64(got).reshape(n_seq, L, heads * dh)[b, :n]
        w = max(w, worst(g, ref[b], np.repeat(tol[b], dh)[None, :]))
    return w


def pool_mean_tolerance(hidden, lens, L):
    h = np.abs(f64(hidden))
    h = h.reshape(-1, L, h.shape[-1])
    return np.stack([n * 2.0 ** -24 * h[b, :n].sum(0) for b, n in enumerate(clamp_lens(lens, L))])


def pool_mean_worst(got, hidden, lens, L):
    tol = pool_mean_tolerance(hidden, lens, L)
    return worst(got, pool_mean(hidden, lens, L, False), np.where(tol > 0, tol, 2.0 ** -150))   # (a zero column is exact)


# ---------------------------------------------------------------------------------------------------- designed inputs: LN
LN_HIDDEN = (64, 128, 512, 576, 1024)     # 8 live lanes; one chunk of 16 lanes; chunk 0 full; 8 lanes of chunk 1; both full
LN_ROWS = (1, 3, 4, 5, 7)                 # four rows share a workgroup
LN_EPS = (1e-12, 1e-5)                    # BERT, MPNet
LN_INPUTS = ("random", "constant", "large_mean", "spike", "full_range", "column_dependent")
EMBED_TOKENS, EMBED_SEQ_LEN, EMBED_VOCAB = (1, 5, 7), 3, 11


def h16(a):
    return np.asarray(a, np.float64).astype(np.float16)


def ln_input(kind, rows, H, seed=0):
    """x, resid [rows][H], gamma, beta [H], all fp16"""
    rng = np.random.default_rng([seed, rows, H, LN_INPUTS.index(kind)])
    gamma, beta = h16(1 + rng.uniform(-0.2, 0.2, H)), h16(rng.standard_normal(H) * 0.1)
    zero = np.zeros((rows, H))
    if kind == "random":
        x, resid = rng.standard_normal((rows, H)), rng.standard_normal((rows, H))
    elif kind == "constant":            # sum and mean exact in fp32: x - mean is 0 and the output is beta on the bits
        x, resid = zero + 0.5, zero
    elif kind == "large_mean":          # the fp16 grid has a step of 0.5 at 1000
        x, resid = 1000 + rng.integers(-1, 2, (rows, H)) * 0.5, rng.standard_normal((rows, H)) * 0.25
    elif kind == "spike":               # one column of 60000 (an fp16 number), in another lane and chunk for every row
        x, resid = zero.copy(), zero
        x[np.arange(rows), (H - 1 + 61 * np.arange(rows)) % H] = 60000
    elif kind == "full_range":          # the sum leaves the fp16 range, fp32 holds it
        x, resid = rng.choice([-30000.0, 30000.0], (rows, H)), rng.choice([-30000.0, 30000.0], (rows, H))
    elif kind == "column_dependent":    # a column permutation across lanes or chunks shows
        x, resid = rng.standard_normal((rows, H)), rng.standard_normal((rows, H))
        gamma, beta = h16(1 + np.arange(H) / H), h16(-np.arange(H) / H)
    else:
        raise ValueError(kind)
    return h16(x), h16(resid), gamma, beta


def embed_input(kind, n_tokens, H, seed=0):
    """ids [n_tokens] (with -1 and vocab: clamped to rows 0 and vocab - 1), word [vocab][H], pos [seq_len][H], type0, gamma, beta"""
    word, _, gamma, beta = ln_input(kind, EMBED_VOCAB, H, seed)
    _, pos, _, _ = ln_input(kind, EMBED_SEQ_LEN, H, seed + 1)
    rng = np.random.default_rng([seed, H, 77])
    type0 = h16(rng.standard_normal(H) * 0.1) if kind in ("random", "column_dependent") else np.zeros(H, np.float16)
    ids = np.array([-1, EMBED_VOCAB, 0, EMBED_VOCAB - 1, 3, 7, 5], np.int32)[:n_tokens]
    return ids, word, pos, type0, gamma, beta


# --------------------------------------------------------------------------------------------- designed inputs: attention
ATTN_L = (1, 31, 32, 33, 63, 64, 65)      # per-wave kernel up to 32, the shared kernel beyond
ATTN_HEADS = {64: 2, 32: 3}               # head_dim -> heads


def boundary_lens(L):
    """1, L - 1, L and every multiple of 32 with its two neighbours, as far as they fit"""
    c = {1, L - 1, L} | {m + d for m in range(32, L + 2, 32) for d in (-1, 0, 1)}
    return np.array(sorted(n for n in c if 1 <= n <= L), np.int32)


def attn_random(lens, L, heads, dh, padding="poison", seed=0):
    """randn * 1.5 on the real rows; rows >= lens[b] of Q, K and V hold +-65504 ("poison", finite on purpose: 0 * inf would
    be NaN in a reference too) or zeros ("zero").  The real rows do not depend on `padding`."""
    n_seq, H = len(lens), heads * dh
    rng = np.random.default_rng([seed, L, heads, dh])
    qkv = (rng.standard_normal((n_seq, L, 3 * H)) * 1.5).astype(np.float16)
    fill = rng.choice([-F16_MAX, F16_MAX], (n_seq, L, 3 * H)).astype(np.float16)
    for b, n in enumerate(lens):
        qkv[b, n:] = fill[b, n:] if padding == "poison" else 0
    return qkv.reshape(n_seq * L, 3 * H)


def _fused(q, k, v):
    """[n_seq][L][heads][dh] each -> [n_seq * L][3 * heads * dh] fp16"""
    n_seq, L = q.shape[:2]
    return np.concatenate([a.reshape(n_seq * L, -1) for a in (q, k, v)], axis=1).astype(np.float16)


def ramp_values(n_seq, L, heads, dh):
    """V[j][d] = (j + d + head) mod 37: whole numbers that depend on the key.  37 is no divisor of a tile, so leaving the last
    tile out (1 to 32 keys) moves an ascending ramp's answer by that many units modulo 37, never by 0."""
    j, d, h = np.arange(L)[:, None, None], np.arange(dh)[None, None, :], np.arange(heads)[None, :, None]
    return np.broadcast_to(((j + d + h) % 37).astype(np.float64), (n_seq, L, heads, dh))


def attn_ramp(lens, L, heads, dh, direction, step=0.5):
    """Q is one constant direction and key j's score is +-step * j (exactly, for head_dim 64; within fp16 rounding of the keys
    for head_dim 32).  Ascending: the running maximum moves in every tile and every rescale is exp(-32 * step).  Descending:
    the maximum sits in tile 0 and the later p run down through the fp16 subnormals to 0."""
    n_seq = len(lens)
    q = np.ones((n_seq, L, heads, dh))
    kj = direction * step * np.arange(L) / np.sqrt(dh)                     # score = sum_d q k / sqrt(dh) = sqrt(dh) * k
    k = np.broadcast_to(kj[None, :, None, None], (n_seq, L, heads, dh))
    return _fused(q, k, ramp_values(n_seq, L, heads, dh))


def attn_peaked(lens, L, heads, dh, where, seed=0):
    """the key at `where` ("first", "last": the last real key, "last_tile": the first key of the last 32-key tile) scores
    about 60 above all others (which score 0); returns qkv and the peak's key index per sequence"""
    n_seq = len(lens)
    rng = np.random.default_rng([seed, L, dh, 3])
    peak = np.array([{"first": 0, "last": n - 1, "last_tile": (n - 1) // 32 * 32}[where] for n in lens])
    q = np.full((n_seq, L, heads, dh), 2.5)
    k = np.zeros((n_seq, L, heads, dh))
    k[np.arange(n_seq), peak] = float(np.float16(60 / (2.5 * np.sqrt(dh))))
    v = rng.standard_normal((n_seq, L, heads, dh)) * 2
    return _fused(q, k, v), peak


def attn_uniform(lens, L, heads, dh, seed=0):
    """K = 0: every real key weighs the same and the output is the mean of the real V rows; V = randn + the tile's number, so a
    tile that is left out or counted twice moves the mean"""
    n_seq = len(lens)
    rng = np.random.default_rng([seed, L, dh, 4])
    q = rng.standard_normal((n_seq, L, heads, dh))
    v = rng.standard_normal((n_seq, L, heads, dh)) + (np.arange(L) // 32 % 4)[None, :, None, None]
    return _fused(q, np.zeros_like(q), v)


def attn_large_scores(lens, L, heads, dh, seed=0):
    """q and k entries of +-11: scores are multiples of 121 * 2 / sqrt(dh), exact in fp32.  Every other key is +- query 0, so
    query 0 scores +-121 sqrt(dh) there (968 at head_dim 64, 684 at 32); the rest are random (|score| up to ~450).  exp
    overflows unless the maximum is subtracted first."""
    n_seq = len(lens)
    rng = np.random.default_rng([seed, L, dh, 5])
    q, k = (rng.choice([-11.0, 11.0], (n_seq, L, heads, dh)) for _ in range(2))
    k[:, ::2] = q[:, :1] * rng.choice([-1.0, 1.0], (n_seq, (L + 1) // 2, heads, 1))
    return _fused(q, k, rng.standard_normal((n_seq, L, heads, dh)) * 2)


# ------------------------------------------------------------------------------------------------- designed inputs: pools
POOL_HIDDEN_MEAN = (8, 64, 136, 1024)
POOL_HIDDEN_CLS = POOL_HIDDEN_MEAN + (2048,)
POOL_POISON = 60000.0


def pool_input(n_seq, L, H, lens, seed=0):
    """randn rows; rows >= the clamped lens[b] hold 60000, so a mean over the wrong span is far outside any tolerance"""
    rng = np.random.default_rng([seed, L, H])
    h = rng.standard_normal((n_seq, L, H))
    for b, n in enumerate(clamp_lens(lens, L)):
        h[b, n:] = POOL_POISON
    return h.astype(np.float16).reshape(n_seq * L, H)


def pool_wide_range_input(n_seq, L, H, seed=0):
    """rows whose squares span 2^-20 .. 2^20: |x| = 2^e with e uniform in [-10, 10], random signs and significands"""
    rng = np.random.default_rng([seed, L, H, 9])
    x = rng.uniform(1, 2, (n_seq, L, H)) * 2.0 ** rng.integers(-10, 10, (n_seq, L, H)) * rng.choice([-1.0, 1.0], (n_seq, L, H))
    return x.astype(np.float16).reshape(n_seq * L, H)
