"""Text handling of HipQwen3Embeddings (encapsulation/embeddings/hip_qwen3.py) with a fake LM that records the id and mask
arrays it is handed — what sentence-transformers does for a decoder embedder: newline -> space, prompt + text tokenised,
truncated to max_length - 1 ids, EOS appended, LEFT padded, batches cut by length.  No GPU."""
import json

import numpy as np
import pytest
import torch

from rag_arc_amd.encapsulation.embeddings.hip_qwen3 import HipQwen3Embeddings

EOS = 999


def tok(text):
    """One id per character, position independent: tok(a + b) == tok(a) + tok(b)."""
    return [5 + ord(c) % 900 for c in text]


class FakeLM:
    """embed_last(ids, mask) -> an embedding that depends on the row's REAL tokens only."""
    hidden, device = 8, "cpu"

    def __init__(self):
        self.calls = []

    def embed_last(self, ids, mask, dim=None, normalize=True):
        ids, mask = np.asarray(ids), np.asarray(mask)
        self.calls.append((ids.copy(), mask.copy(), dim, normalize))
        out = np.zeros((ids.shape[0], dim or self.hidden), np.float32)
        for r in range(ids.shape[0]):
            real = ids[r][mask[r].astype(bool)]
            out[r] = [float((real * (c + 1)).sum() % 1009) + len(real) for c in range(out.shape[1])]
        return torch.from_numpy(out)

    def rows(self):
        """Every real-token sequence the LM saw, over all calls."""
        return [ids[r][mask[r].astype(bool)].tolist() for ids, mask, _, _ in self.calls for r in range(ids.shape[0])]


def test_newlines_prompt_and_eos():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, prompt="P: ", eos_token_id=EOS)
    emb.embed_documents(["a\nb\n"])
    assert lm.rows() == [tok("P: a b ") + [EOS]]
    ids, mask, dim, normalize = lm.calls[0]
    assert dim is None and normalize is True and ids.dtype == np.int32


def test_query_prompt_is_used_by_the_query_methods_only():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, prompt="D ", query_prompt="Q\n", eos_token_id=EOS)
    emb.embed_documents(["x"])
    emb.embed_query("x\ny")
    emb.embed_queries(["z"])
    emb.embed_queries_device(["w"])
    emb.embed_documents_device(["v"])
    # (the newline of the PROMPT stays: only the texts are cleaned, as huggingface.py:116 does before encode() prepends it)
    assert lm.rows() == [tok("D x") + [EOS], tok("Q\nx y") + [EOS], tok("Q\nz") + [EOS], tok("Q\nw") + [EOS], tok("D v") + [EOS]]
    lm2 = FakeLM()
    one = HipQwen3Embeddings(lm2, tok, prompt="D ", eos_token_id=EOS)        # no query prompt: one prompt serves both
    one.embed_query("x")
    assert lm2.rows() == [tok("D x") + [EOS]]


def test_eos_is_appended_after_truncation():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, prompt="ab", max_length=6, eos_token_id=EOS)
    emb.embed_documents(["cdefghij", "c"])
    rows = sorted(lm.rows(), key=len)
    assert rows == [tok("abc") + [EOS], tok("abcde") + [EOS]]            # 5 = max_length - 1 ids, then EOS: 6 in all
    lm = FakeLM()
    HipQwen3Embeddings(lm, tok, max_length=6, append_eos=False).embed_documents(["cdefghij"])
    assert lm.rows() == [tok("cdefgh")]


def test_left_padding_and_the_empty_string():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, eos_token_id=EOS, pad_id=3)
    out = emb.embed_documents(["abcd", "", "xy"])
    assert len(out) == 3 and all(len(v) == 8 for v in out)
    ids, mask, _, _ = lm.calls[0]
    assert len(lm.calls) == 1 and ids.shape == (3, 5)
    assert (ids[:, -1] == EOS).all() and (mask[:, -1] == 1).all()         # the last position is every row's EOS
    assert mask.tolist() == [[1, 1, 1, 1, 1], [0, 0, 1, 1, 1], [0, 0, 0, 0, 1]]   # longest first, pads on the left
    assert ids[2].tolist() == [3, 3, 3, 3, EOS] and ids[1].tolist() == [3, 3] + tok("xy") + [EOS]
    # ... and the results come back in the order of the texts
    lm2 = FakeLM()
    assert HipQwen3Embeddings(lm2, tok, eos_token_id=EOS).embed_documents([""]) == [out[1]]
    assert lm2.rows() == [[EOS]]


def test_batches_are_cut_by_length():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, eos_token_id=EOS, batch_tokens=256)
    texts = ["a" * n for n in (3, 200, 5, 90, 7, 60, 1, 2)]
    out = emb.embed_documents(texts)
    shapes = [c[0].shape for c in lm.calls]
    # longest first; a call holds batch_tokens // (its longest, rounded up to 32) rows: 256 // 224, 256 // 96, 256 // 32
    assert shapes == [(1, 201), (2, 91), (5, 8)]
    assert emb.last_stats["lm_calls"] == 3 and emb.last_stats["tokens"] == sum(len(t) + 1 for t in texts)
    assert emb.last_stats["padded_tokens"] == 224 + 2 * 96 + 5 * 32 < 8 * 224     # not padded to the longest text
    alone = [HipQwen3Embeddings(FakeLM(), tok, eos_token_id=EOS).embed_documents([t])[0] for t in texts]
    assert out == alone                                                   # un-permuted: row i belongs to text i


def test_query_equals_first_document_when_the_prompts_coincide():
    for kw in ({}, {"prompt": "same "}, {"prompt": "same ", "query_prompt": "same "}):
        emb = HipQwen3Embeddings(FakeLM(), tok, eos_token_id=EOS, **kw)
        for t in ("hello\nworld", ""):
            assert emb.embed_query(t) == emb.embed_documents([t])[0] == emb.embed_queries([t])[0]


def test_dim_and_normalize_reach_the_lm():
    lm = FakeLM()
    emb = HipQwen3Embeddings(lm, tok, dim=4, normalize=False, eos_token_id=EOS)
    assert len(emb.embed_query("q")) == 4 and lm.calls[0][2:] == (4, False)
    assert emb.embed_documents([]) == [] and emb.embed_documents_device([]).shape == (0, 4)
    with pytest.raises(ValueError):
        HipQwen3Embeddings(lm, tok, dim=9)
    with pytest.raises(ValueError):
        HipQwen3Embeddings(lm, tok, dim=0)


class FakePrefixLM(FakeLM):
    """... with the prefix hooks: records the prefix batch and the remainders."""

    def __init__(self):
        super().__init__()
        self.prefixes, self.rests = [], []

    def prefix_kv_device(self, d_ids, d_start):
        self.prefixes.append((d_ids.numpy().copy(), d_start.numpy().copy()))
        return {"n": d_ids.shape[0], "P": d_ids.shape[1]}

    def embed_last_device(self, d_ids, d_start, dim=None, normalize=True, out=None, prefix=None, prefix_of=None):
        ids, start = d_ids.numpy(), d_start.numpy()
        assert prefix is not None and (prefix_of.numpy() == 0).all() and (ids.shape[0] * ids.shape[1]) % 128 == 0
        self.rests.append([ids[r, start[r]:].tolist() for r in range(ids.shape[0])])
        return torch.zeros((ids.shape[0], dim or self.hidden))


def test_prefix_cache_runs_the_query_prompt_once(monkeypatch):
    monkeypatch.delenv("RARC_LM_EMBED_PREFIX", raising=False)
    prompt = "Instruct: retrieve passages\nQuery:"                       # 34 tokens >= 16
    lm = FakePrefixLM()
    emb = HipQwen3Embeddings(lm, tok, query_prompt=prompt, eos_token_id=EOS, prefix_cache=True)
    emb.embed_queries(["abc", ""])
    emb.embed_query("de")
    assert len(lm.prefixes) == 1                                          # lazily, once
    pre, pstart = lm.prefixes[0]
    assert pre.shape == (4, 64) and pre[0, 64 - 34:].tolist() == tok(prompt) and pstart.tolist() == [30, 63, 63, 63]
    assert lm.rests[0][:2] == [tok("abc") + [EOS], [EOS]]                 # the empty text: the EOS alone
    assert lm.rests[1][0] == tok("de") + [EOS] and not lm.calls
    assert emb.last_stats["prefix_tokens"] == 34
    emb.embed_documents(["abc"])                                          # documents: the plain call, always
    assert len(lm.calls) == 1 and len(lm.rests) == 2
    # switched off: by the environment, by the constructor (the default), by a prompt under 16 tokens
    monkeypatch.setenv("RARC_LM_EMBED_PREFIX", "0")
    emb.embed_query("x")
    assert len(lm.calls) == 2 and len(lm.rests) == 2
    monkeypatch.delenv("RARC_LM_EMBED_PREFIX")
    for kw in ({"query_prompt": prompt}, {"query_prompt": "short:", "prefix_cache": True}):
        lm2 = FakePrefixLM()
        HipQwen3Embeddings(lm2, tok, eos_token_id=EOS, **kw).embed_query("x")
        assert len(lm2.calls) == 1 and not lm2.rests
    monkeypatch.setenv("RARC_LM_EMBED_PREFIX", "1")                       # ... and on, for an A/B run of the default
    lm3 = FakePrefixLM()
    HipQwen3Embeddings(lm3, tok, query_prompt=prompt, eos_token_id=EOS).embed_query("x")
    assert not lm3.calls and len(lm3.rests) == 1


def test_prefix_cache_steps_aside_when_the_seam_merges():
    """A tokenizer that merges across the prompt / text seam: prompt + text does not begin with the prompt's own tokens, so
    the batch takes the plain call (same tokens as without the cache)."""
    prompt = "p" * 20

    def merging(text):
        return [7] * (len(text) // 2) + tok(text[len(text) // 2 * 2:])      # pairs of characters become one token

    lm = FakePrefixLM()
    emb = HipQwen3Embeddings(lm, lambda t: tok(t) if t == prompt else merging(t), query_prompt=prompt, eos_token_id=EOS,
                             prefix_cache=True)
    emb.embed_query("abc")
    assert len(lm.calls) == 1 and not lm.rests and lm.rows() == [merging(prompt + "abc") + [EOS]]


def test_json_registry_round_trip(tmp_path, monkeypatch):
    """JSON -> Register.register -> HipQwen3Embeddings with every argument of the config (the LM itself replaced by the fake:
    no GPU here), and the same config nested as a store's `embedding`."""
    from tokenizers import Tokenizer, models, pre_tokenizers

    import rag_arc_amd.core.rerank.hip_qwen3 as lm_mod
    from rag_arc_amd.config.app_registration import register_qwen3_embeddings, registrator
    from rag_arc_amd.config.modules import HipFlatVectorStoreConfig, HipQwen3EmbeddingsConfig

    words = ["<|endoftext|>", "[UNK]", "query", ":", "a", "vector", "index"]
    t = Tokenizer(models.WordLevel({w: i for i, w in enumerate(words)}, unk_token="[UNK]"))
    t.pre_tokenizer = pre_tokenizers.Whitespace()
    t.save(str(tmp_path / "tokenizer.json"))
    np.savez(tmp_path / "model.npz", **{"norm.weight": np.ones(8, np.float32)})
    seen = {}

    class Stub(FakeLM):
        def __init__(self, sd, nq, nkv, dh, **kw):
            super().__init__()
            seen.update(keys=sorted(sd), heads=(nq, nkv, dh), kw=kw)

    monkeypatch.setattr(lm_mod, "HipCausalLM", Stub)
    cfg = {"type": "hip_qwen3_embeddings", "weights_path": str(tmp_path / "model.npz"), "tokenizer_path": str(tmp_path / "tokenizer.json"),
           "num_attention_heads": 16, "num_key_value_heads": 8, "head_dim": 128, "tie_word_embeddings": False,
           "prompt": "", "query_prompt": "query : ", "dim": 4, "normalize": False, "max_length": 12, "batch_tokens": 4096}
    (tmp_path / "emb.json").write_text(json.dumps(cfg))
    register_qwen3_embeddings(str(tmp_path / "emb.json"), "q3e")
    mod = registrator.get_object("q3e")
    emb = mod.impl
    assert isinstance(emb, HipQwen3Embeddings) and mod.config.type == "hip_qwen3_embeddings"
    assert seen["heads"] == (16, 8, 128) and seen["kw"]["tie_word_embeddings"] is False and seen["keys"] == ["norm.weight"]
    assert (emb.dim, emb.normalize, emb.max_length, emb.batch_tokens, emb.query_prompt) == (4, False, 12, 4096, "query : ")
    assert emb.eos_token_id == 0 and emb.append_eos                      # <|endoftext|> looked up in the tokenizer
    assert len(mod.embed_query("a vector index")) == 4                   # the module forwards to the provider
    assert emb.lm.rows() == [[2, 3, 4, 5, 6, 0]]
    nested = HipFlatVectorStoreConfig(**{"type": "hip_flat_vectorstore", "embedding": cfg})
    assert isinstance(nested.embedding, HipQwen3EmbeddingsConfig) and nested.embedding.dim == 4
    with pytest.raises(ValueError, match="hip_qwen3_embeddings"):
        HipQwen3EmbeddingsConfig(**{**cfg, "tokenizer_path": None}).build()
