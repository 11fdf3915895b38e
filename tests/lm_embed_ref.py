"""Reference side of the decoder-LM embedding tests (tests/test_gpu_lm_embed.py, tests/test_lm_embed_host.py).

The fp32 reference needs no forward of its own: oracle.qwen3_last_logits_f32 honours an untied head, and with
lm_head = I (rows 0 .. H-1 of a [vocab][H] table) and token_ids = 0 .. H-1 its "logits" ARE the final-normed last hidden
state, exactly (a product with 0 / 1 entries).  Truncation and normalisation are done here in float64."""
import numpy as np


def identity_head(vocab: int, hidden: int) -> np.ndarray:
    """[vocab][hidden], row c = e_c for c < hidden (vocab >= hidden): logit of token c = component c of the normed state."""
    assert vocab >= hidden
    return np.eye(vocab, hidden, dtype=np.float32)


def fp16_weights(sd) -> dict:
    """The weights as the device holds them (rounded to fp16), widened again for the fp32 oracle."""
    return {k: np.asarray(v, np.float32).astype(np.float16).astype(np.float32) for k, v in sd.items()}


def last_hidden_f32(oracle, sd16, cfg, input_ids, attention_mask) -> np.ndarray:
    """fp32 [n][H]: RMSNorm(final) of the last position's residual row — what Pooling(lasttoken) hands to Normalize."""
    hidden = int(np.asarray(sd16["model.norm.weight"]).shape[0])
    vocab = int(np.asarray(sd16["model.embed_tokens.weight"]).shape[0])
    sd = dict(sd16)
    sd["lm_head.weight"] = identity_head(vocab, hidden)
    return oracle.qwen3_last_logits_f32(sd, cfg, input_ids, attention_mask, np.arange(hidden))


def truncate_normalize_f64(x, dim=None, normalize=True) -> np.ndarray:
    """sentence-transformers' truncate_dim then Normalize, in float64: x[:, :dim] / max(||x[:, :dim]||, 1e-12)."""
    x = np.asarray(x, dtype=np.float64)
    x = x if dim is None else x[:, :dim]
    if not normalize:
        return x
    return x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True)), 1e-12)


def rel_err(got, want) -> float:
    """Worst per-component error relative to the row's rms component."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rms = np.sqrt((want * want).mean(axis=1, keepdims=True))
    return float((np.abs(got - want) / rms).max())


def one_minus_cos(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    cos = (got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))
    return float((1.0 - cos).max())


def last_only(n_seq: int, seq_len: int, hidden: int, n_q: int, head_dim: int, inter: int) -> bool:
    """The condition under which lm_forward (csrc/decoder.hip) runs the last layer on the last positions only, for the
    batch HipCausalLM makes of [n_seq][seq_len] host arrays (length padded to a multiple of 32, rows to a multiple of 4)."""
    L = -(-seq_len // 32) * 32
    n = -(-n_seq // 4) * 4
    T, Mp, QD = n * L, -(-n // 128) * 128, n_q * head_dim
    return 6 * 256 + Mp * (QD + 3 * hidden + 3 * inter) * 2 <= T * 2 * inter * 2
