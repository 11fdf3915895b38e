"""The encoder's layer pieces alone, through the C-ABI, against the float64 references of tests/enc_ref.py at the widths, row
counts, lengths and inputs where they can go wrong while the whole forward's end-to-end tolerance notices nothing
(rarc_enc_embed_ln, rarc_enc_add_ln, rarc_enc_attention, rarc_enc_pool, rarc_enc_pool_mean).  The tolerances are those derived
in tests/enc_ref.py; whatever is claimed to hold on the bits is compared on the bits.  Every output buffer starts as NaN with
one guard row behind it that must stay NaN."""
import numpy as np
import pytest

from tests import enc_ref as R

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _lib():
    from rag_arc_amd.hip import binding as B

    return B, B.load_library()


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _guarded(rows, cols, dtype):
    import torch

    return torch.full((rows + 1, cols), NAN, dtype=dtype, device="cuda")


def _result(out, rows):
    import torch

    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert np.isnan(o[rows]).all(), "the guard row behind the output was written"
    return o[:rows]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


# ------------------------------------------------------------------------------------------------------------ a. LayerNorm
def _add_ln(x, resid, gamma, beta, eps, in_place=False):
    import torch

    B, lib = _lib()
    rows, H = x.shape
    out = _guarded(rows, H, torch.float16)
    dx, dg, db = _dev(x), _dev(gamma), _dev(beta)
    if in_place:                                             # as the forward calls it: rarc_enc_add_ln(y, x, ..., x)
        out[:rows] = _dev(resid)
        dr = out
    else:
        dr = _dev(resid)
    B.check(lib.rarc_enc_add_ln(dx.data_ptr(), dr.data_ptr(), dg.data_ptr(), db.data_ptr(), eps, rows, H, out.data_ptr(), _stream()),
            "rarc_enc_add_ln")
    return _result(out, rows)


def _embed_ln(ids, word, pos, type0, gamma, beta, eps):
    import torch

    B, lib = _lib()
    n, H = len(ids), word.shape[1]
    out = _guarded(n, H, torch.float16)
    d = [_dev(a) for a in (ids, word, pos, type0, gamma, beta)]
    B.check(lib.rarc_enc_embed_ln(*[t.data_ptr() for t in d], eps, n, R.EMBED_SEQ_LEN, H, R.EMBED_VOCAB, out.data_ptr(), _stream()),
            "rarc_enc_embed_ln")
    return _result(out, n)


def _check_ln(got, z, gamma, beta, eps, kind, what):
    assert np.isfinite(R.f64(got)).all(), what
    w = R.ln_worst(got, z, gamma, beta, eps)
    assert w <= 1.0, f"{what}: |got - ref| is {w:.3f} of the tolerance"
    if kind == "constant":                                   # x - mean is exactly 0: beta on the bits, though rstd is 1e6 at eps 1e-12
        assert np.array_equal(bits(got), bits(np.broadcast_to(beta, got.shape))), what
    return w


@pytest.mark.parametrize("H", R.LN_HIDDEN)
def test_add_ln_at_every_lane_mask_and_row_count(H):
    worst = 0.0
    for kind in R.LN_INPUTS:
        for rows in R.LN_ROWS:
            x, resid, gamma, beta = R.ln_input(kind, rows, H)
            z = R.f64(x) + R.f64(resid)
            for eps in R.LN_EPS:
                what = f"add_ln {kind} H={H} rows={rows} eps={eps}"
                got = _add_ln(x, resid, gamma, beta, eps)
                worst = max(worst, _check_ln(got, z, gamma, beta, eps, kind, what))
                same = _add_ln(x, resid, gamma, beta, eps, in_place=True)
                assert np.array_equal(bits(same), bits(got)), what + ": in place differs from out of place"
    print(f"add_ln H={H}: worst |got - ref| / tolerance = {worst:.3f}")


@pytest.mark.parametrize("H", R.LN_HIDDEN)
def test_embed_ln_at_every_lane_mask_and_token_count(H):
    worst = 0.0
    for kind in R.LN_INPUTS:
        for n in R.EMBED_TOKENS:                             # seq_len 3: t % seq_len wraps inside a workgroup of four tokens
            ids, word, pos, type0, gamma, beta = R.embed_input(kind, n, H)
            z = R.embed_sum(ids, word, pos, type0, R.EMBED_SEQ_LEN)
            for eps in R.LN_EPS:
                got = _embed_ln(ids, word, pos, type0, gamma, beta, eps)
                worst = max(worst, _check_ln(got, z, gamma, beta, eps, kind, f"embed_ln {kind} H={H} tokens={n} eps={eps}"))
    print(f"embed_ln H={H}: worst |got - ref| / tolerance = {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------ b. attention
def _attention(qkv, lens, L, heads, dh):
    import torch

    B, lib = _lib()
    n_seq, H = len(lens), heads * dh
    assert qkv.shape == (n_seq * L, 3 * H) and qkv.dtype == np.float16
    ctx = _guarded(n_seq * L, H, torch.float16)
    dq, dl = _dev(qkv), _dev(np.asarray(lens, np.int32))
    B.check(lib.rarc_enc_attention(dq.data_ptr(), dl.data_ptr(), n_seq, L, H, heads, ctx.data_ptr(), _stream()), "rarc_enc_attention")
    return _result(ctx, n_seq * L)


def _check_attention(got, qkv, lens, L, heads, dh, what):
    n_seq = len(lens)
    ref = R.attention(qkv, lens, n_seq, L, heads, dh)
    w = R.attention_worst(got, ref, qkv, lens, n_seq, L, heads, dh)
    assert w <= 1.0, f"{what}: |got - ref| is {w:.3f} of 2^-9 max|V|"
    return w


def _real_rows(a, lens, L):
    a = a.reshape(len(lens), L, -1)
    return np.concatenate([a[b, :n] for b, n in enumerate(lens)])


def _cases():
    """(L, lens): the per-wave kernel (L <= 32), the shared one beyond, and 512 keys with a ragged last tile"""
    return [(L, R.boundary_lens(L)) for L in (32, 33, 65)] + [(512, np.array([509], np.int32))]


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("L", R.ATTN_L + (512,))
def test_attention_at_boundary_lengths_ignores_poisoned_padding(L, dh):
    """rows >= lens[b] of Q, K and V hold +-65504: the real rows come out as with zeros there, on the bits"""
    heads, lens = (R.ATTN_HEADS[dh], R.boundary_lens(L)) if L < 512 else (1, np.array([509], np.int32))
    qkv = R.attn_random(lens, L, heads, dh, "poison")
    got = _attention(qkv, lens, L, heads, dh)
    w = _check_attention(got, qkv, lens, L, heads, dh, f"L={L} dh={dh}")
    clean = _attention(R.attn_random(lens, L, heads, dh, "zero"), lens, L, heads, dh)
    assert np.array_equal(bits(_real_rows(got, lens, L)), bits(_real_rows(clean, lens, L))), "padding rows reached a real row"
    print(f"attention L={L} dh={dh} lens={lens.tolist()}: worst / tolerance = {w:.3f}")


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("direction", [+1, -1])
def test_attention_on_score_ramps(direction, dh):
    """ascending: the maximum moves in every tile and the rescale is exp(-16) (steep) or exp(-2) (gentle, every tile counts);
    descending: the maximum sits in tile 0 and p runs down through the fp16 subnormals"""
    for L, lens in _cases():
        heads = R.ATTN_HEADS[dh] if L < 512 else 1
        for step in (0.5, 1 / 16):
            qkv = R.attn_ramp(lens, L, heads, dh, direction, step)
            w = _check_attention(_attention(qkv, lens, L, heads, dh), qkv, lens, L, heads, dh, f"ramp {direction:+d} step={step} L={L} dh={dh}")
            print(f"attention ramp {direction:+d} step={step} L={L} dh={dh}: worst / tolerance = {w:.3f}")


@pytest.mark.parametrize("dh", [64, 32])
def test_attention_peaked_uniform_and_large_scores(dh):
    for L, lens in _cases():
        heads = R.ATTN_HEADS[dh] if L < 512 else 1
        n_seq = len(lens)
        for where in ("first", "last", "last_tile"):
            qkv, peak = R.attn_peaked(lens, L, heads, dh, where)
            got = _attention(qkv, lens, L, heads, dh)
            _check_attention(got, qkv, lens, L, heads, dh, f"peak {where} L={L} dh={dh}")
            v = R.f64(qkv).reshape(n_seq, L, 3, heads * dh)[:, :, 2]
            for b, n in enumerate(lens):                     # the peak's V row, to within the output's one rounding
                want = v[b, peak[b]][None, :]
                assert np.all(np.abs(R.f64(got).reshape(n_seq, L, -1)[b, :n] - want) <= 2.0 ** -11 * np.abs(want) + 2.0 ** -25), (where, L, b)
        for make in (R.attn_uniform, R.attn_large_scores):
            qkv = make(lens, L, heads, dh)
            _check_attention(_attention(qkv, lens, L, heads, dh), qkv, lens, L, heads, dh, f"{make.__name__} L={L} dh={dh}")


# ------------------------------------------------------------------------------------------------------------ c, d. pools
def _pool(hidden, n_seq, L, normalize, lens=None):
    import torch

    B, lib = _lib()
    H = hidden.shape[1]
    out = _guarded(n_seq, H, torch.float32)
    dh_ = _dev(hidden)
    if lens is None:
        B.check(lib.rarc_enc_pool(dh_.data_ptr(), n_seq, L, H, normalize, out.data_ptr(), _stream()), "rarc_enc_pool")
    else:
        dl = _dev(np.asarray(lens, np.int32))
        B.check(lib.rarc_enc_pool_mean(dh_.data_ptr(), dl.data_ptr(), n_seq, L, H, normalize, out.data_ptr(), _stream()), "rarc_enc_pool_mean")
    return _result(out, n_seq)


def _l2norm(rows):
    import torch

    B, lib = _lib()
    n, H = rows.shape
    src, out = _dev(rows), _guarded(n, H, torch.float32)
    B.check(lib.rarc_l2norm_rows_f32(src.data_ptr(), H, out.data_ptr(), H, n, H, _stream()), "rarc_l2norm_rows_f32")
    return _result(out, n)


def _pool_lens(L):
    mid = (L + 1) // 2
    return [np.array([1, L, mid], np.int32), np.array([0, L + 3, mid], np.int32)]      # the second: clamped to 1 and L


@pytest.mark.parametrize("H", R.POOL_HIDDEN_CLS)
def test_cls_pooling_is_exact_and_normalises_in_the_canonical_order(H):
    for L in (1, 5):
        for hid in (R.pool_input(3, L, H, [1, 1, 1]), R.pool_wide_range_input(3, L, H)):   # (every row behind the first: 60000)
            raw = _pool(hid, 3, L, 0)
            assert np.array_equal(bits(raw), bits(hid.reshape(3, L, H)[:, 0].astype(np.float32))), (H, L)
            assert np.array_equal(bits(_pool(hid, 3, L, 1)), bits(_l2norm(raw))), (H, L)
    zero = np.zeros((3 * 5, H), np.float16)
    zero[1:5] = R.POOL_POISON
    assert not _pool(zero, 3, 5, 1).any()                    # zero rows stay zero: no NaN from 1 / sqrt(0)


@pytest.mark.parametrize("H", R.POOL_HIDDEN_MEAN)
def test_mean_pooling_over_the_real_tokens_only(H):
    for L in (1, 5):
        for lens in _pool_lens(L):
            for hid in (R.pool_input(3, L, H, lens), R.pool_wide_range_input(3, L, H)):
                raw = _pool(hid, 3, L, 0, lens)
                w = R.pool_mean_worst(raw, hid, lens, L)
                assert w <= 1.0, f"H={H} L={L} lens={lens.tolist()}: |got - ref| is {w:.3f} of len 2^-24 sum|x|"
                assert np.array_equal(bits(_pool(hid, 3, L, 1, lens)), bits(_l2norm(raw))), (H, L, lens.tolist())
    zero = np.zeros((3 * 5, H), np.float16)
    zero[2:5] = R.POOL_POISON
    assert not _pool(zero, 3, 5, 1, [2, 5, 1]).any()


# ------------------------------------------------------------------------------------------------- e. pieces equal the whole
def _encoder(oracle, H, layers, heads, I, seed, pooling):
    from rag_arc_amd.encapsulation.embeddings.hip_bert import HipBertEncoder

    sd = oracle.random_bert_state_dict(H, layers, heads, I, vocab=50, max_pos=32, seed=seed)
    return HipBertEncoder(sd, num_heads=heads, pooling=pooling, precision="fp16")


def _by_hand(enc, d_ids, d_lens, normalize):
    """the forward of csrc/encoder.hip, piece by piece through the ABI; also what entered the last LayerNorm (y, resid, mid)"""
    import torch

    B, lib = _lib()
    n_seq, L = d_ids.shape
    M, H, I, st = n_seq * L, enc.hidden, enc.inter, _stream()
    new = lambda cols: torch.full((M, cols), NAN, dtype=torch.float16, device="cuda")
    x, y, ctx, qkv, mid = new(H), new(H), new(H), new(3 * H), new(I)
    p = lambda t: t.data_ptr()
    gemm = lambda a, w, b, c, n, k, act: B.check(lib.rarc_enc_gemm(p(a), p(w), p(b), p(c), M, n, k, act, st), "rarc_enc_gemm")
    add_ln = lambda g, b: B.check(lib.rarc_enc_add_ln(p(y), p(x), p(g), p(b), enc.eps, M, H, p(x), st), "rarc_enc_add_ln")
    B.check(lib.rarc_enc_embed_ln(p(d_ids), p(enc.word), p(enc.pos), p(enc.type0), p(enc.emb_g), p(enc.emb_b), enc.eps, M, L, H,
                                  enc.vocab, p(x), st), "rarc_enc_embed_ln")
    last = None
    for i, w in enumerate(enc.layers):
        gemm(x, w["qkv_w"], w["qkv_b"], qkv, 3 * H, H, 0)
        B.check(lib.rarc_enc_attention(p(qkv), p(d_lens), n_seq, L, H, enc.heads, p(ctx), st), "rarc_enc_attention")
        gemm(ctx, w["o_w"], w["o_b"], y, H, H, 0)
        add_ln(w["ln1_g"], w["ln1_b"])
        gemm(x, w["f1_w"], w["f1_b"], mid, I, H, 1)
        gemm(mid, w["f2_w"], w["f2_b"], y, H, I, 0)
        if i == len(enc.layers) - 1:
            last = tuple(t.cpu().numpy() for t in (y, x, mid))
        add_ln(w["ln2_g"], w["ln2_b"])
    out = torch.full((n_seq, H), NAN, dtype=torch.float32, device="cuda")
    if enc._pool_bit:
        B.check(lib.rarc_enc_pool_mean(p(x), p(d_lens), n_seq, L, H, normalize, p(out), st), "rarc_enc_pool_mean")
    else:
        B.check(lib.rarc_enc_pool(p(x), n_seq, L, H, normalize, p(out), st), "rarc_enc_pool")
    torch.cuda.synchronize()
    return out.cpu().numpy(), last


def _batch():
    rng = np.random.default_rng(3)
    lens = np.array([32, 1, 17, 31], np.int32)
    ids = rng.integers(1, 50, (4, 32)).astype(np.int32)
    for b, n in enumerate(lens):
        ids[b, n:] = 0
    return _dev(ids), _dev(lens), lens


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_the_pieces_chained_by_hand_are_the_forward_on_the_bits(oracle, pooling):
    """H = 128, I = 256, 128 tokens: no GEMM is split (k / 2 < 8 * 64), so rarc_enc_forward issues exactly these calls"""
    enc = _encoder(oracle, 128, 2, 2, 256, 11, pooling)
    d_ids, d_lens, _ = _batch()
    for normalize in (0, 1):
        whole = enc.forward_device(d_ids, d_lens, normalize=bool(normalize)).cpu().numpy()
        hand, _ = _by_hand(enc, d_ids, d_lens, normalize)
        assert np.isfinite(hand).all() and np.array_equal(bits(hand), bits(whole)), (pooling, normalize)


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_the_split_k_layernorm_agrees_with_the_unsplit_chain(oracle, pooling):
    """I = 2048 splits FFN2 four ways: the forward's LayerNorm kernel sums fp32 partials (n_parts > 0), reachable in no other way.
    One layer, no normalisation, so that this LayerNorm is the last thing in front of the pool and everything before it is the
    by-hand chain's on the bits.  Bound, per token and column (then through the pool: the CLS row itself, or the mean over the
    real tokens plus both means' own summation error):
      the two y = fp16(bias + sum of products) round fp32 sums taken in different orders.  Either sum is within
      e = (K + 1) 2^-24 (sum_k |a_k w_k| + |bias|) of the exact one (products of fp16 numbers are exact in fp32), so the two y are
      at most d = ulp16(y) + 2e apart; D = max_j d_j over the row.
      LayerNorm of z and z + delta, |delta_j| <= D: the mean moves by <= D, z_j - mean by <= 2D; var moves by
      <= 2 sqrt(var) D, so rstd by <= rstd^2 D relatively (first order; the factor 1 + 4 D rstd covers the second):
          |delta out_j| <= |gamma_j| rstd D (2 + |zhat_j|) (1 + 4 D rstd),   zhat = (z - mean) rstd
      and each side is within enc_ref.ln_tolerance of the exact LayerNorm of its own z."""
    enc = _encoder(oracle, 128, 1, 2, 2048, 12, pooling)
    d_ids, d_lens, lens = _batch()
    whole = enc.forward_device(d_ids, d_lens, normalize=False).cpu().numpy()
    hand, (y, resid, mid) = _by_hand(enc, d_ids, d_lens, 0)
    w = enc.layers[0]
    W, bias, gamma, beta = (R.f64(w[k].cpu().numpy()) for k in ("f2_w", "f2_b", "ln2_g", "ln2_b"))
    K = W.shape[1]
    e = (K + 1) * 2.0 ** -24 * (np.abs(R.f64(mid)) @ np.abs(W).T + np.abs(bias))
    D = (R.f64(np.spacing(np.abs(y))) + 2 * e).max(-1, keepdims=True)
    z = R.f64(y) + R.f64(resid)
    mean = z.mean(-1, keepdims=True)
    rstd = 1 / np.sqrt(((z - mean) ** 2).mean(-1, keepdims=True) + enc.eps)
    ref = R.layer_norm(z, gamma, beta, enc.eps)
    bound = np.abs(gamma) * rstd * D * (2 + np.abs(z - mean) * rstd) * (1 + 4 * D * rstd) + 2 * R.ln_tolerance(z, gamma, enc.eps, ref)
    bound = bound.reshape(4, 32, -1)
    if pooling == "cls":
        bound = bound[:, 0]
    else:
        hid = ref.reshape(128, -1)
        bound = np.stack([bound[b, :n].mean(0) for b, n in enumerate(lens)]) + 2 * R.pool_mean_tolerance(hid, lens, 32)
    ratio = R.worst(whole, R.f64(hand), bound)
    print(f"split-K LayerNorm, {pooling}: worst |forward - chain| / bound = {ratio:.3f}, differing elements {int((whole != hand).sum())}")
    assert ratio <= 1.0
