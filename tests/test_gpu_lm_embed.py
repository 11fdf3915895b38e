"""Decoder-LM embeddings on the GPU: rarc_lm_embed_last / _prefixed (csrc/decoder.hip: the reranker's forward ending in
rarc_lm_last_embed_kernel) through HipCausalLM.embed_last*, HipQwen3Embeddings and a store.  Seeded weights
(oracle.random_qwen3_state_dict) at geometries of tests/test_gpu_reranker_lm.py.

Which ending of lm_forward a geometry takes (the `last_only` condition, lm_embed_ref.last_only restates it; the batch is
padded to rows % 4 == 0, length % 32 == 0 first):
    A  5 x 40 -> 512 tokens, Mp 128:  656 896 <=  1 048 576   compact branch (last layer on the last rows; stride 1, offset 0)
    B  4 x 32 -> 128 tokens:          460 288 >     131 072   full branch (stride seq_len, offset seq_len - 1)
    C  8 x 64 -> 512 tokens:        3 671 552 <=  6 291 456   compact branch
    D 32 x 64 -> 2048 tokens:       1 836 544 <= 16 777 216   compact branch
    E  5 x 24 -> 256 tokens (A's model): 656 896 > 524 288    full branch, head_dim 64, ragged padding
test_both_endings_are_covered asserts exactly this table.

Measured on an MI355X (worst per-component error relative to the row's rms component, against the fp32 oracle):
see the docstring of test_against_the_fp32_reference."""
import functools

import numpy as np
import pytest

from tests import lm_embed_ref as R

pytestmark = pytest.mark.gpu

#        H, layers, n_q, n_kv, head_dim, ffn, n, L, pads
GEO = {
    "A": (256, 2, 4, 2, 64, 512, 5, 40, (0, 7, 33, 39, 16)),
    "B": (256, 1, 2, 2, 128, 256, 4, 32, (0, 31, 1, 12)),
    "C": (1024, 2, 16, 8, 128, 3072, 8, 64, (0, 5, 20, 63)),
    "D": (256, 2, 4, 2, 64, 2048, 32, 64, (0,)),
    "E": (256, 2, 4, 2, 64, 512, 5, 24, (0, 7, 23, 12, 1)),
}
VOCAB = 1280          # >= every H: the identity head has a row per component


def _cfg(g):
    H, LAYERS, NQ, NKV, DH, I = GEO[g][:6]
    return dict(num_attention_heads=NQ, num_key_value_heads=NKV, head_dim=DH, rms_norm_eps=1e-6, rope_theta=1e6)


def yardstick(lm_id, ids, mask, want):
    """The parent's path on the same weights and inputs: yes_no_logits through the identity head returns half(nv[c0]),
    half(nv[c1]) — every component of the final-normed last state, two per forward.  Returns (fp16 values [n][H] as fp32,
    their worst error relative to the row's rms component against `want`)."""
    H = want.shape[1]
    z = np.empty(want.shape, np.float32)
    for c in range(0, H, 2):
        z[:, c:c + 2] = lm_id.yes_no_logits(ids, mask, c, c + 1).float().cpu().numpy()
    return z, R.rel_err(z, want)


@functools.lru_cache(maxsize=None)
def case(g):
    """Model (identity head), inputs, the fp32 reference and the yardstick of one geometry — computed once, never modified."""
    from oracle import cpu_ref as oracle
    from rag_arc_amd.core.rerank import HipCausalLM

    H, LAYERS, NQ, NKV, DH, I, n, L, pads = GEO[g]
    sd = oracle.random_qwen3_state_dict(H, LAYERS, NQ, NKV, DH, I, vocab=VOCAB, seed=H + L)
    sd["lm_head.weight"] = R.identity_head(VOCAB, H)
    lm = HipCausalLM(sd, NQ, NKV, DH, rms_norm_eps=1e-6, rope_theta=1e6)
    rng = np.random.default_rng(H + L)
    ids = rng.integers(5, VOCAB, (n, L))
    mask = np.ones((n, L), np.int64)
    for r in range(n):
        p = pads[r % len(pads)]
        mask[r, :p] = 0
        ids[r, :p] = 0
    want = R.last_hidden_f32(oracle, R.fp16_weights(sd), _cfg(g), ids, mask)
    z, e_y = yardstick(lm, ids, mask, want)
    raw = lm.embed_last(ids, mask, normalize=False).cpu().numpy()
    for a in (ids, mask, want, z, raw):
        a.setflags(write=False)
    return dict(sd=sd, lm=lm, ids=ids, mask=mask, want=want, z=z, e_y=e_y, raw=raw, H=H)


def test_both_endings_are_covered():
    got = {g: R.last_only(v[6], v[7], v[0], v[2], v[4], v[5]) for g, v in GEO.items()}
    assert got == {"A": True, "B": False, "C": True, "D": True, "E": False}


@pytest.mark.parametrize("g", list(GEO))
def test_unnormalised_output_is_the_logit_path_bit_for_bit(g):
    """Identity head: the unchanged yes_no_logits returns half(nv[c0]), half(nv[c1]); embed_last(normalize=False) must return
    the same halves, widened, at those components — eight pairs per geometry, components 0 and H - 1 among them."""
    c = case(g)
    H, raw = c["H"], c["raw"]
    assert raw.dtype == np.float32 and raw.shape == (c["ids"].shape[0], H) and np.isfinite(raw).all()
    rng = np.random.default_rng(H)
    pairs = [(0, H - 1), (H - 1, 0), (1, H - 2), (H // 2, H // 2 - 1)] + [tuple(int(v) for v in rng.integers(0, H, 2)) for _ in range(4)]
    for c0, c1 in pairs:
        z = c["lm"].yes_no_logits(c["ids"], c["mask"], c0, c1).cpu().numpy()
        assert z.dtype == np.float16
        mine = raw[:, [c0, c1]]
        assert np.array_equal(mine.astype(np.float16).astype(np.float32), mine)          # exactly representable halves
        assert np.array_equal(mine.astype(np.float16).view(np.uint16), z.view(np.uint16)), (g, c0, c1)
    # (the yardstick of test 3 went through every component the same way)
    assert np.array_equal(raw.astype(np.float16).view(np.uint16), c["z"].astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("g", list(GEO))
def test_normalisation(g):
    """out = nv / max(||nv[:dim]||, 1e-12) against float64 normalisation of the call's OWN un-normalised output:
    |d| <= (dim + 4) * 2^-24 — an fp32 sum of dim squares (relative error <= dim * 2^-24 on the sum, half of it on its
    root), one square root, one maximum, one division (2^-24 relative each), on components of magnitude <= 1."""
    c = case(g)
    H = c["H"]
    for dim in (H, H // 2, 64):
        got = c["lm"].embed_last(c["ids"], c["mask"], dim=dim, normalize=True).cpu().numpy()
        assert got.shape == (c["ids"].shape[0], dim) and got.dtype == np.float32
        want = R.truncate_normalize_f64(c["raw"], dim)
        d = np.abs(got - want).max()
        print(f"LM-EMBED-NORM {g} dim={dim}: max|d|={d:.2e} (bound {(dim + 4) * 2.0 ** -24:.2e})")
        assert d <= (dim + 4) * 2.0 ** -24
        un = c["lm"].embed_last(c["ids"], c["mask"], dim=dim, normalize=False).cpu().numpy()
        assert np.array_equal(un, c["raw"][:, :dim])                                       # truncation alone: a prefix of the row


def test_an_all_zero_row_gives_zeros_not_nan():
    from rag_arc_amd.core.rerank import HipCausalLM

    c = case("B")
    H, LAYERS, NQ, NKV, DH, I = GEO["B"][:6]
    sd = dict(c["sd"])
    sd["model.norm.weight"] = np.zeros(H, np.float32)
    lm = HipCausalLM(sd, NQ, NKV, DH, rms_norm_eps=1e-6, rope_theta=1e6)
    for normalize in (True, False):
        out = lm.embed_last(c["ids"], c["mask"], normalize=normalize).cpu().numpy()
        assert out.shape == (4, H) and (out == 0).all()


def test_ld_out_larger_than_out_dim_leaves_the_gap_untouched():
    import torch

    c = case("B")                                  # 4 x 32 = 128 tokens: goes to the device entry as it is
    lm, H = c["lm"], c["H"]
    d_ids = torch.from_numpy(c["ids"].astype(np.int32)).to(lm.device)
    d_start = torch.from_numpy((c["mask"] == 0).sum(1).astype(np.int32)).to(lm.device)
    for dim, ld in ((H, H + 7), (64, 100)):
        buf = torch.full((4, ld), -7.5, dtype=torch.float32, device=lm.device)
        out = lm.embed_last_device(d_ids, d_start, dim=dim, normalize=False, out=buf)
        assert out.shape == (4, dim) and out.data_ptr() == buf.data_ptr()
        host = buf.cpu().numpy()
        assert np.array_equal(host[:, :dim], c["raw"][:, :dim]) and (host[:, dim:] == -7.5).all()
    with pytest.raises(ValueError):
        lm.embed_last_device(d_ids, d_start, dim=64, out=torch.empty((4, 63), dtype=torch.float32, device=lm.device))
    with pytest.raises(ValueError):
        lm.embed_last_device(d_ids, d_start, dim=H + 1)


def test_a_checkpoint_without_a_head_embeds_and_refuses_logits():
    """Qwen3Model names (no "model." prefix), no lm_head.weight, untied: constructs, embeds the same bits (prefix cache
    included), and the logits methods say why they cannot answer."""
    import torch

    from rag_arc_amd.core.rerank import HipCausalLM
    from rag_arc_amd.hip import binding as B

    c = case("B")
    H, LAYERS, NQ, NKV, DH, I = GEO["B"][:6]
    bare = {k[len("model."):]: v for k, v in c["sd"].items() if k != "lm_head.weight"}
    lm = HipCausalLM(bare, NQ, NKV, DH, rms_norm_eps=1e-6, rope_theta=1e6, tie_word_embeddings=False)
    assert lm.lm_head is None
    assert np.array_equal(lm.embed_last(c["ids"], c["mask"], normalize=False).cpu().numpy(), c["raw"])
    with pytest.raises(B.RarcError, match="no lm_head"):
        lm.yes_no_logits(c["ids"], c["mask"], 1, 2)
    d_ids = torch.from_numpy(c["ids"].astype(np.int32)).to(lm.device)
    d_start = torch.from_numpy((c["mask"] == 0).sum(1).astype(np.int32)).to(lm.device)
    with pytest.raises(B.RarcError, match="no lm_head"):
        lm.yes_no_logits_device(d_ids, d_start, 1, 2)
    handle = lm.prefix_kv_device(d_ids, d_start)                                   # the prefix cache needs no head either
    both = [m.embed_last_device(d_ids, d_start, prefix=handle, prefix_of=torch.tensor([0, -1, 2, 3], dtype=torch.int32, device=lm.device))
            for m in (lm, c["lm"])]
    assert torch.isfinite(both[0]).all() and torch.equal(both[0], both[1])


@pytest.mark.parametrize("g", list(GEO))
def test_against_the_fp32_reference(g):
    """Error against the fp32 oracle (same fp16-rounded weights), per component relative to the row's rms component, and
    1 - cos.  The yardstick is the parent's yes_no_logits path on the same weights and inputs through the identity head
    (existing code, measured here: e_y); the un-normalised embedding IS that path's output, the normalised one gets
    2 x e_y, because the norm it divides by carries the same error once more.

    Measured on an MI355X (e_y = yardstick; normalised embedding at dim = H and H / 2; worst 1 - cos):
        A  e_y 4.26e-3   normalised 4.24e-3 / 3.69e-3   1 - cos 9.9e-7
        B  e_y 3.24e-3   normalised 3.23e-3 / 2.99e-3   1 - cos 4.2e-7
        C  e_y 7.48e-3   normalised 7.46e-3 / 6.02e-3   1 - cos 1.7e-6
        D  e_y 6.01e-3   normalised 6.00e-3 / 5.52e-3   1 - cos 1.8e-6
        E  e_y 4.67e-3   normalised 4.63e-3 / 4.53e-3   1 - cos 1.2e-6
    (test_prefixed_against_plain, same unit: A yardstick 4.80e-3, prefixed vs oracle 5.34e-3, vs plain 5.69e-3;
     C yardstick 7.09e-3, prefixed vs oracle 6.78e-3, vs plain 7.68e-3.)"""
    c = case(g)
    H, e_y = c["H"], c["e_y"]
    e_raw = R.rel_err(c["raw"], c["want"])
    assert e_raw == e_y                                                   # the same bits (test 1), so the same error
    assert e_y > 0                                                        # an fp16 forward against an fp32 one: not nothing
    for dim in (H, H // 2):
        got = c["lm"].embed_last(c["ids"], c["mask"], dim=dim, normalize=True).cpu().numpy()
        want = R.truncate_normalize_f64(c["want"], dim)
        e_n, omc = R.rel_err(got, want), R.one_minus_cos(got, want)
        print(f"LM-EMBED-REF {g} dim={dim}: yardstick e_y={e_y:.3e}  normalised e={e_n:.3e} (bound {2 * e_y:.3e})  1-cos={omc:.2e}")
        assert e_n <= 2 * e_y


def _tok(text):
    """One id per character, position independent: tok(prompt + text) == tok(prompt) + tok(text)."""
    return [5 + (ord(ch) * 7) % 1200 for ch in text]


EOS = 1279


@pytest.mark.parametrize("g", ["A", "C"])
def test_prefixed_against_plain(g, monkeypatch):
    """A 20-token shared prompt, remainders of 1 (the EOS alone: an empty text) to 60 tokens, through the provider: with the
    prefix cache (rarc_lm_prefix_kv once, rarc_lm_embed_last_prefixed per batch) and without.  One tolerance for both
    relations, the one of test_against_the_fp32_reference with the yardstick measured on THESE inputs: prefixed against the
    oracle on the whole prompts, and prefixed against plain."""
    from oracle import cpu_ref as oracle
    from rag_arc_amd.encapsulation.embeddings.hip_qwen3 import HipQwen3Embeddings

    monkeypatch.delenv("RARC_LM_EMBED_PREFIX", raising=False)
    c = case(g)
    lm, H = c["lm"], c["H"]
    prompt = "Instruct: find it. Q"                                       # 20 characters = 20 tokens
    assert len(_tok(prompt)) == 20
    lens = [0, 1, 2, 5, 9, 17, 30, 31, 32, 45, 58, 59]                    # + EOS: remainders of 1 .. 60 tokens
    texts = ["".join(chr(97 + (i * 5 + j * 3) % 26) for j in range(n)) for i, n in enumerate(lens)]
    full = [_tok(prompt + t) + [EOS] for t in texts]
    L = max(map(len, full))
    ids, mask = np.zeros((len(full), L), np.int64), np.zeros((len(full), L), np.int64)
    for r, f in enumerate(full):
        ids[r, L - len(f):] = f
        mask[r, L - len(f):] = 1
    want_raw = R.last_hidden_f32(oracle, R.fp16_weights(c["sd"]), _cfg(g), ids, mask)
    _, e_y = yardstick(lm, ids, mask, want_raw)
    want = R.truncate_normalize_f64(want_raw)
    with_cache = HipQwen3Embeddings(lm, _tok, query_prompt=prompt, eos_token_id=EOS, prefix_cache=True)
    without = HipQwen3Embeddings(lm, _tok, query_prompt=prompt, eos_token_id=EOS, prefix_cache=False)
    pre = with_cache.embed_queries_device(texts).cpu().numpy()
    assert with_cache.last_stats["prefix_tokens"] == 20 and with_cache.last_stats["tokens"] == sum(lens) + len(lens)
    plain = without.embed_queries_device(texts).cpu().numpy()
    assert without.last_stats["prefix_tokens"] == 0 and without.last_stats["tokens"] == sum(map(len, full))
    e_pre, e_plain, e_pp = R.rel_err(pre, want), R.rel_err(plain, want), R.rel_err(pre, plain)
    print(f"LM-EMBED-PREFIX {g}: yardstick e_y={e_y:.3e} (bound {2 * e_y:.3e}); prefixed vs oracle {e_pre:.3e}, plain vs oracle "
          f"{e_plain:.3e}, prefixed vs plain {e_pp:.3e}; 1-cos prefixed vs oracle {R.one_minus_cos(pre, want):.2e}")
    assert np.isfinite(pre).all() and e_pre <= 2 * e_y and e_plain <= 2 * e_y and e_pp <= 2 * e_y
    assert e_pp > 0                                                        # the prefixed kernels did run (another summation order)
    one = with_cache.embed_query("")                                       # the EOS alone, alone
    assert R.rel_err(np.asarray([one]), want[:1]) <= 2 * e_y


def test_provider_fills_and_queries_a_store():
    """HipFlatVectorStore(HipQwen3Embeddings) over 300 synthetic texts through add_texts: the device hook is taken (no
    vector visits the host), and 20 of the stored texts, queried with the same prompt, each come back at rank 1 with
    score >= 1 - 1e-3.  (A query is embedded in a batch padded differently from its ingest batch, and the store keeps fp16
    rows: both are 1e-3-class perturbations of the COMPONENTS, second order in the cosine.)"""
    from rag_arc_amd.encapsulation.database.vector_db.hip_flat import HipFlatVectorStore
    from rag_arc_amd.encapsulation.embeddings.hip_qwen3 import HipQwen3Embeddings

    lm = case("A")["lm"]
    emb = HipQwen3Embeddings(lm, _tok, prompt="passage: ", eos_token_id=EOS, batch_tokens=4096)
    taken = []
    hook = emb.embed_documents_device
    emb.embed_documents_device = lambda texts: (taken.append(len(texts)), hook(texts))[1]
    rng = np.random.default_rng(300)
    texts = [f"text {i} " + "".join(chr(97 + int(v)) for v in rng.integers(0, 26, int(rng.integers(1, 90)))) for i in range(300)]
    store = HipFlatVectorStore(emb, metric="cosine")
    ids = store.add_texts(texts, ids=[str(i) for i in range(300)])
    assert taken == [300] and store.ntotal == 300 and len(ids) == 300
    assert emb.last_stats["lm_calls"] > 1                                  # several length buckets, not one padded batch
    picks = [int(v) for v in rng.choice(300, 20, replace=False)]
    scores = []
    for i in picks:
        (doc, score), = store.similarity_search_with_score(texts[i], k=1)
        assert doc.id == str(i) and doc.content == texts[i], (i, doc.id)
        scores.append(score)
    print(f"LM-EMBED-STORE: min score of 20 self-queries {min(scores):.6f}")
    assert min(scores) >= 1 - 1e-3
    batch = store.batch_similarity_search_with_score([texts[i] for i in picks], k=1)          # embed_queries_device
    assert [b[0][0].id for b in batch] == [str(i) for i in picks] and min(b[0][1] for b in batch) >= 1 - 1e-3
