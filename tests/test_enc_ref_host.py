"""tests/enc_ref.py without a GPU: (1) its float64 stages, chained with plain matmuls and erf-GELU, are the forward the project
already trusts (oracle.bert_forward_f32 in float64, to 1e-10); (2) its comparators can fail: on the designed inputs of
tests/test_gpu_encoder_pieces.py, with the reference standing in for the kernel, each of a set of small planted errors is
rejected and the unmodified reference passes."""
import numpy as np
import pytest

from tests import enc_ref as R


# ------------------------------------------------------------------------------------------------------ the reference chain
def _chain(sd, ids, lens, heads, eps, pooling, normalize):
    from scipy.special import erf

    g = lambda k: np.asarray(sd[k], np.float32).astype(np.float64)
    n_seq, L = ids.shape
    H = g("embeddings.word_embeddings.weight").shape[1]
    x = R.embed_ln(ids.reshape(-1), g("embeddings.word_embeddings.weight"), g("embeddings.position_embeddings.weight"),
                   g("embeddings.token_type_embeddings.weight")[0], g("embeddings.LayerNorm.weight"), g("embeddings.LayerNorm.bias"),
                   eps, L)
    i = 0
    while f"encoder.layer.{i}.attention.self.query.weight" in sd:
        p = f"encoder.layer.{i}."
        w = np.concatenate([g(p + f"attention.self.{n}.weight") for n in ("query", "key", "value")])
        b = np.concatenate([g(p + f"attention.self.{n}.bias") for n in ("query", "key", "value")])
        real = R.attention(x @ w.T + b, lens, n_seq, L, heads, H // heads)
        ctx = np.zeros((n_seq, L, H))                         # (padding queries reach no real token's output: left at 0)
        for s, rows in enumerate(real):
            ctx[s, :len(rows)] = rows
        y = ctx.reshape(-1, H) @ g(p + "attention.output.dense.weight").T + g(p + "attention.output.dense.bias")
        x = R.add_ln(y, x, g(p + "attention.output.LayerNorm.weight"), g(p + "attention.output.LayerNorm.bias"), eps)
        h = x @ g(p + "intermediate.dense.weight").T + g(p + "intermediate.dense.bias")
        h = 0.5 * h * (1.0 + erf(h / np.sqrt(2.0)))
        y = h @ g(p + "output.dense.weight").T + g(p + "output.dense.bias")
        x = R.add_ln(y, x, g(p + "output.LayerNorm.weight"), g(p + "output.LayerNorm.bias"), eps)
        i += 1
    return R.pool_mean(x, lens, L, normalize) if pooling == "mean" else R.pool_cls(x, L, normalize)


@pytest.mark.parametrize("heads", [2, 4])                    # head_dim 64 and 32
def test_the_chained_references_are_the_float64_oracle(oracle, heads):
    sd = oracle.random_bert_state_dict(128, 2, heads, 256, vocab=60, max_pos=16, seed=heads)
    rng = np.random.default_rng(heads)
    ids = rng.integers(0, 60, (5, 9)).astype(np.int32)
    lens = np.array([9, 1, 4, 8, 2])
    for pooling in ("cls", "mean"):
        for normalize in (True, False):
            want = oracle.bert_forward_f32(sd, ids, lens, heads, eps=1e-12, normalize=normalize, pooling=pooling, dtype=np.float64)
            got = _chain(sd, ids, lens, heads, 1e-12, pooling, normalize)
            assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-10, (pooling, normalize)


def test_lens_and_ids_are_clamped_as_the_kernels_clamp_them():
    assert R.clamp_lens([0, -3, 5, 9], 5).tolist() == [1, 1, 5, 5]
    word = np.arange(8.0).reshape(4, 2)
    z = R.embed_sum([-1, 4, 2], word, np.zeros((2, 2)), np.zeros(2), 2)
    assert np.array_equal(z, word[[0, 3, 2]])
    assert R.boundary_lens(65).tolist() == [1, 31, 32, 33, 63, 64, 65] and R.boundary_lens(1).tolist() == [1]
    assert R.boundary_lens(33).tolist() == [1, 31, 32, 33] and R.boundary_lens(512)[-4:].tolist() == [480, 481, 511, 512]


# ------------------------------------------------------------------------------------------------- the comparators can fail
def _away(got16, ref, idx):
    """got16[idx] moved by one fp16 ulp, away from ref"""
    out = got16.copy()
    out[idx] = np.nextafter(got16[idx], np.float16(np.inf if float(got16[idx]) >= ref[idx] else -np.inf))
    return out


@pytest.mark.parametrize("H", R.LN_HIDDEN)
@pytest.mark.parametrize("kind", ["random", "column_dependent"])
def test_one_fp16_ulp_in_one_layernorm_output_is_rejected(H, kind):
    """On rows without cancellation the fp32 term is far below an ulp, so the tolerance is the output's one rounding: the
    correctly rounded reference passes, and the same array with ONE element one ulp further from the reference does not.  (The
    element is one whose reference lies in the lower half of its binade and is at least 2^-3: there an ulp, 2^-10 of the
    binade's lower end, is more than 4/3 of 2^-11 |ref|, whatever the first rounding did.)"""
    for eps in R.LN_EPS:
        x, resid, gamma, beta = R.ln_input(kind, 5, H)
        z = R.f64(x) + R.f64(resid)
        ref = R.layer_norm(z, gamma, beta, eps)
        got = ref.astype(np.float16)
        assert R.ln_worst(got, z, gamma, beta, eps) <= 1.0
        frac = np.abs(ref) / 2.0 ** np.floor(np.log2(np.maximum(np.abs(ref), 1e-30)))
        cand = np.argwhere((np.abs(ref) >= 0.125) & (frac < 1.5))
        assert len(cand)
        for idx in (tuple(cand[0]), tuple(cand[-1])):
            assert R.ln_worst(_away(got, ref, idx), z, gamma, beta, eps) > 1.0, (eps, idx)


@pytest.mark.parametrize("kind", R.LN_INPUTS)
def test_layernorm_reference_passes_its_own_comparator_on_every_designed_input(kind):
    for H in R.LN_HIDDEN:
        for eps in R.LN_EPS:
            x, resid, gamma, beta = R.ln_input(kind, 7, H)
            assert x.dtype == resid.dtype == gamma.dtype == beta.dtype == np.float16 and np.isfinite(R.f64(x)).all()
            z = R.f64(x) + R.f64(resid)
            got = R.layer_norm(z, gamma, beta, eps).astype(np.float16)
            assert np.isfinite(R.f64(got)).all() and R.ln_worst(got, z, gamma, beta, eps) <= 1.0
            if kind == "constant":
                assert np.array_equal(got, np.broadcast_to(beta, got.shape))
            ids, word, pos, type0, g2, b2 = R.embed_input(kind, 7, H)
            assert {-1, 0, R.EMBED_VOCAB - 1, R.EMBED_VOCAB} <= set(ids.tolist())
            z = R.embed_sum(ids, word, pos, type0, R.EMBED_SEQ_LEN)
            assert R.ln_worst(R.embed_ln(ids, word, pos, type0, g2, b2, eps, R.EMBED_SEQ_LEN).astype(np.float16), z, g2, b2, eps) <= 1.0


def _as_kernel(ref_rows, n_seq, L, H):
    """a list of real rows -> the fp16 [n_seq * L][H] array a kernel leaves (padding rows: whatever, here NaN)"""
    out = np.full((n_seq, L, H), np.nan, np.float16)
    for b, rows in enumerate(ref_rows):
        out[b, :len(rows)] = rows.astype(np.float16)
    return out.reshape(n_seq * L, H)


@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("L", [L for L in R.ATTN_L if L > 1])
def test_a_mask_that_is_off_by_one_key_is_rejected(L, dh):
    """lens + 1 lets the first padding key in: with poisoned padding (K, V = +-65504 there) on the boundary lengths"""
    heads, lens = R.ATTN_HEADS[dh], R.boundary_lens(L)
    n_seq = len(lens)
    qkv = R.attn_random(lens, L, heads, dh, "poison")
    ref = R.attention(qkv, lens, n_seq, L, heads, dh)
    assert R.attention_worst(_as_kernel(ref, n_seq, L, heads * dh), ref, qkv, lens, n_seq, L, heads, dh) <= 1.0
    wrong = [rows[:n] for rows, n in zip(R.attention(qkv, lens + 1, n_seq, L, heads, dh), lens)]
    assert R.attention_worst(wrong, ref, qkv, lens, n_seq, L, heads, dh) > 1.0
    for b in range(n_seq - 1):                                # a sequence with a padding key, taken alone, is rejected too
        if lens[b] < 8:                                       # (a handful of rows: the poisoned key's score may be negative in all)
            continue
        one = [wrong[i] if i == b else ref[i] for i in range(n_seq)]
        assert R.attention_worst(one, ref, qkv, lens, n_seq, L, heads, dh) > 1.0, int(lens[b])
    # the real rows do not depend on the padding
    assert np.array_equal(R.attention(R.attn_random(lens, L, heads, dh, "zero"), lens, n_seq, L, heads, dh)[0], ref[0])


def _online(qkv, lens, n_seq, L, heads, dh, rescale=True, tile=32):
    """the online softmax over 32-key tiles in float64; rescale=False forgets to rescale the ACCUMULATOR when the maximum moves"""
    q, k, v = R.split_qkv(qkv, n_seq, L, heads, dh)
    out = []
    for b, n in enumerate(R.clamp_lens(lens, L)):
        m, l, o = np.full((heads, n, 1), -np.inf), np.zeros((heads, n, 1)), np.zeros((heads, n, dh))
        for k0 in range(0, n, tile):
            s = q[b, :, :n] @ k[b, :, k0:min(n, k0 + tile)].transpose(0, 2, 1) / np.sqrt(dh)
            m_new = np.maximum(m, s.max(-1, keepdims=True))
            corr, p = np.exp(m - m_new), np.exp(s - m_new)
            l = l * corr + p.sum(-1, keepdims=True)
            o = o * (corr if rescale else 1.0) + p @ v[b, :, k0:min(n, k0 + tile)]
            m = m_new
        out.append((o / l).transpose(1, 0, 2).reshape(n, heads * dh))
    return out


@pytest.mark.parametrize("dh", [64, 32])
def test_an_accumulator_that_is_not_rescaled_is_rejected_on_the_ascending_ramp(dh):
    heads = R.ATTN_HEADS[dh]
    for L in (33, 65, 512):
        lens = R.boundary_lens(L) if L < 512 else np.array([509], np.int32)
        lens = lens[lens > 32]                                # (one tile: nothing to rescale)
        n_seq = len(lens)
        for step in (0.5, 1 / 16):
            qkv = R.attn_ramp(lens, L, heads, dh, +1, step)
            ref = R.attention(qkv, lens, n_seq, L, heads, dh)
            good = _online(qkv, lens, n_seq, L, heads, dh)
            assert max(np.max(np.abs(a - b)) for a, b in zip(good, ref)) <= 1e-12
            assert R.attention_worst(_as_kernel(ref, n_seq, L, heads * dh), ref, qkv, lens, n_seq, L, heads, dh) <= 1.0
            bad = _online(qkv, lens, n_seq, L, heads, dh, rescale=False)
            for b in range(n_seq):
                one = [bad[i] if i == b else ref[i] for i in range(n_seq)]
                assert R.attention_worst(one, ref, qkv, lens, n_seq, L, heads, dh) > 1.0, (L, step, int(lens[b]))


@pytest.mark.parametrize("dh", [64, 32])
def test_the_other_designed_attention_inputs_pass_and_say_what_they_claim(dh):
    heads, L = R.ATTN_HEADS[dh], 65
    lens = R.boundary_lens(L)
    n_seq = len(lens)
    for where in ("first", "last", "last_tile"):              # the output is the peak's V row
        qkv, peak = R.attn_peaked(lens, L, heads, dh, where)
        v = R.split_qkv(qkv, n_seq, L, heads, dh)[2]
        for b, rows in enumerate(R.attention(qkv, lens, n_seq, L, heads, dh)):
            assert np.max(np.abs(rows - v[b, :, peak[b]].reshape(-1))) <= 1e-20
    qkv = R.attn_uniform(lens, L, heads, dh)                  # the output is the mean of the real V rows
    v = R.split_qkv(qkv, n_seq, L, heads, dh)[2]
    for b, rows in enumerate(R.attention(qkv, lens, n_seq, L, heads, dh)):
        assert np.max(np.abs(rows - v[b, :, :lens[b]].mean(1).reshape(-1))) <= 1e-12
    qkv = R.attn_large_scores(lens, L, heads, dh)             # scores near 1e3 at head_dim 64: exp(score) alone overflows fp32
    q, k, _ = R.split_qkv(qkv, n_seq, L, heads, dh)
    top = np.abs(q[-1] @ k[-1].transpose(0, 2, 1)).max() / np.sqrt(dh)
    assert np.isclose(top, 121 * np.sqrt(dh)) and top > 88 and np.all(np.isfinite(np.concatenate(R.attention(qkv, lens, n_seq, L, heads, dh))))
    qkv = R.attn_ramp(lens, L, heads, dh, -1)                 # descending: p falls below the smallest fp16 subnormal inside tile 1
    assert 0.5 * 63 > -np.log(2.0 ** -25)
    ref = R.attention(qkv, lens, n_seq, L, heads, dh)
    assert R.attention_worst(_as_kernel(ref, n_seq, L, heads * dh), ref, qkv, lens, n_seq, L, heads, dh) <= 1.0


@pytest.mark.parametrize("H", R.POOL_HIDDEN_MEAN)
def test_a_mean_over_the_wrong_span_is_rejected(H):
    L, lens = 5, np.array([1, 5, 3, 0, 8], np.int32)           # 0 and 8 are clamped to 1 and 5
    hid = R.pool_input(5, L, H, lens)
    ref = R.pool_mean(hid, lens, L, False)
    assert np.array_equal(ref[3], R.f64(hid)[3 * L]) and R.pool_mean_worst(ref.astype(np.float32), hid, lens, L) <= 1.0
    n = R.clamp_lens(lens, L)
    by_L = np.stack([R.f64(hid).reshape(5, L, H)[b, :n[b]].sum(0) / L for b in range(5)])        # divides by L, not by len
    whole = R.f64(hid).reshape(5, L, H).mean(1)                                                   # averages the padding too
    for wrong in (by_L, whole):
        assert R.pool_mean_worst(wrong.astype(np.float32), hid, lens, L) > 1.0
        for b in (0, 2, 3):                                   # every sequence shorter than L, taken alone
            one = ref.copy()
            one[b] = wrong[b]
            assert R.pool_mean_worst(one.astype(np.float32), hid, lens, L) > 1.0
    # one fp32 ulp is inside the bound only where several tokens were added
    up = np.nextafter(ref.astype(np.float32), np.float32(np.inf))
    assert R.pool_mean_worst(up, hid, lens, L) > 1.0 and np.all(np.abs(up[1] - ref[1]) <= R.pool_mean_tolerance(hid, lens, L)[1])
    assert np.allclose(np.linalg.norm(R.pool_mean(hid, lens, L, True), axis=1), 1) and np.allclose(np.linalg.norm(R.pool_cls(hid, L, True), axis=1), 1)
    assert not R.pool_cls(np.zeros((2, 8)), 1, True).any()      # a zero row stays zero, no NaN
