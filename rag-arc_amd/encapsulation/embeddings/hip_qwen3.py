"""Decoder-LM embedding provider on the MI355X: Qwen3-Embedding (0.6B / 4B / 8B) and its family — what the reference's
HuggingFaceEmbeddings gives for such a checkpoint (core/file_management/embeddings/huggingface.py:96-98,105-145:
`SentenceTransformer(model_name)`, newline -> space, encode, python float lists out).

A sentence-transformers decoder embedder is Transformer -> Pooling(lasttoken) -> Normalize: the causal LM the reranker
already runs (csrc/decoder.hip), ending in the final-normed hidden state of the last token instead of two logits
(rarc_lm_embed_last, include/rarc.h).  Text handling is sentence-transformers' for this family: `prompt + text` is
tokenised with the checkpoint's byte-level BPE (core/rerank/bpe.py), truncated to max_length - 1 ids, the EOS id
(<|endoftext|>) appended, batches LEFT padded so that the last position is every row's EOS.

Precision: fp16 weights, activations and residual stream, fp32 accumulation, fp32 output — the class of the reference's
`model_kwargs={"torch_dtype": float16}` model, not the fp32 class of the BERT path.
"""
from __future__ import annotations

import os
import threading
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .base import Embeddings


class HipQwen3Embeddings(Embeddings):
    """Embeddings provider: tokenizer callable + HipCausalLM (core/rerank/hip_qwen3.py).

    prompt         put in front of EVERY text (sentence-transformers' `prompt`; the reference's embed_query is
                   embed_documents([text])[0], so one prompt serves both)
    query_prompt   extension: when set, the query methods use it instead (Qwen3-Embedding's "Instruct: ...\\nQuery:")
    dim            Matryoshka truncation (truncate_dim): keep the first `dim` components, then normalise
    batch_tokens   padded tokens per LM call; texts are sorted by length first, so a ragged corpus is cut into calls of
                   similar lengths instead of being padded to its longest text
    prefix_cache   run a query prompt of at least MIN_PREFIX_TOKENS tokens through the LM once (prefix_kv_device) and every
                   query batch through the prefixed call, which costs only the queries' own tokens.  None = the class default
                   (DESIGN, "Decoder-LM embeddings": what the measurement said); RARC_LM_EMBED_PREFIX=0 / 1 overrides both."""

    EOS_TOKEN_ID = 151643          # <|endoftext|>: Qwen2 / Qwen3's first added token, the EOS their embedding checkpoints append
    MIN_PREFIX_TOKENS = 16
    PREFIX_CACHE_DEFAULT = False

    def __init__(self, lm, tokenize: Callable[[str], Sequence[int]], prompt: str = "", query_prompt: Optional[str] = None,
                 dim: Optional[int] = None, normalize: bool = True, max_length: int = 4096, batch_tokens: int = 32768,
                 append_eos: bool = True, eos_token_id: int = EOS_TOKEN_ID, pad_id: int = 0,
                 prefix_cache: Optional[bool] = None, **kwargs):
        super().__init__(**kwargs)
        self.lm, self.tokenize = lm, tokenize
        self.prompt, self.query_prompt = prompt or "", query_prompt
        self.dim = None if dim is None else int(dim)
        hidden = getattr(lm, "hidden", None)
        if self.dim is not None and (self.dim < 1 or (hidden is not None and self.dim > hidden)):
            raise ValueError(f"dim must lie in [1, {hidden}]")
        self.normalize = bool(normalize)
        self.max_length = int(max_length)
        if self.max_length < 1:
            raise ValueError("max_length must be at least 1")
        self.batch_tokens = max(128, int(batch_tokens))
        self.append_eos, self.eos_token_id, self.pad_id = bool(append_eos), int(eos_token_id), int(pad_id)
        self.prefix_cache = self.PREFIX_CACHE_DEFAULT if prefix_cache is None else bool(prefix_cache)
        self._prefix = None            # (prompt ids, handle of prefix_kv_device), made at the first prefixed query batch
        self._prefix_lock = threading.Lock()
        self.last_stats: Dict[str, float] = {}

    # -- host side: texts -> token sequences -> left-padded batches -----------------------------------------------------
    def _sequences(self, texts: Sequence[str], prompt: str) -> List[List[int]]:
        room = self.max_length - 1 if self.append_eos else self.max_length
        seqs = []
        for x in texts:
            ids = list(self.tokenize(prompt + x.replace("\n", " ")))[: max(room, 0)]
            if self.append_eos:
                ids.append(self.eos_token_id)
            seqs.append(ids or [self.pad_id])
        return seqs

    def _batches(self, lens: Sequence[int]):
        """Cut a run of sequences sorted LONGEST FIRST into LM calls: as many as fit `batch_tokens` once padded to the call's
        longest (its first; a multiple of 32)."""
        n, s = len(lens), 0
        while s < n:
            longest = -(-int(lens[s]) // 32) * 32
            e = min(n, s + max(1, self.batch_tokens // longest))
            yield s, e
            s = e

    @staticmethod
    def _left_pad(seqs: Sequence[Sequence[int]], pad_id: int):
        L = max(len(s) for s in seqs)
        ids = np.full((len(seqs), L), pad_id, np.int32)
        mask = np.zeros((len(seqs), L), np.int8)
        for r, s in enumerate(seqs):
            ids[r, L - len(s):] = s
            mask[r, L - len(s):] = 1
        return ids, mask

    def _use_prefix(self, prompt: str) -> bool:
        env = os.environ.get("RARC_LM_EMBED_PREFIX")
        on = self.prefix_cache if env is None else env != "0"
        return bool(on and prompt and hasattr(self.lm, "prefix_kv_device"))

    def _prefix_handle(self, prompt: str):
        """(token ids of the query prompt, its K/V rows of every layer) — computed at the first use, then kept."""
        with self._prefix_lock:
            if self._prefix is None or self._prefix[0] != prompt:
                import torch

                pids = list(self.tokenize(prompt))
                handle = None
                if len(pids) >= self.MIN_PREFIX_TOKENS and len(pids) <= 4096:
                    P = -(-len(pids) // 32) * 32                     # one prefix row, left padded; 4 rows make a multiple of 128
                    pre = np.full((4, P), self.pad_id, np.int32)
                    pre[0, P - len(pids):] = pids
                    pstart = np.array([P - len(pids), P - 1, P - 1, P - 1], np.int32)
                    dev = self.lm.device
                    handle = self.lm.prefix_kv_device(torch.from_numpy(pre).to(dev), torch.from_numpy(pstart).to(dev))
                self._prefix = (prompt, pids, handle)
            return self._prefix[1], self._prefix[2]

    # -- the LM calls --------------------------------------------------------------------------------------------------
    def _embed_plain(self, seqs: List[List[int]]):
        ids, mask = self._left_pad(seqs, self.pad_id)
        return self.lm.embed_last(ids, mask, dim=self.dim, normalize=self.normalize)

    def _embed_prefixed(self, rests: List[List[int]], handle):
        import torch

        n = len(rests)
        Ls = -(-max(len(r) for r in rests) // 32) * 32
        n_pad = -(-n // 4) * 4
        ids = np.full((n_pad, Ls), self.pad_id, np.int32)
        start = np.full(n_pad, Ls - 1, np.int32)
        for r, rest in enumerate(rests):
            ids[r, Ls - len(rest):] = rest
            start[r] = Ls - len(rest)
        dev = self.lm.device
        out = self.lm.embed_last_device(torch.from_numpy(ids).to(dev), torch.from_numpy(start).to(dev), dim=self.dim,
                                        normalize=self.normalize, prefix=handle,
                                        prefix_of=torch.zeros(n_pad, dtype=torch.int32, device=dev))
        return out[:n]

    def _embed_device(self, texts: List[str], prompt: str, prefixed: bool):
        import torch

        n = len(texts)
        if n == 0:
            width = self.dim if self.dim is not None else getattr(self.lm, "hidden", 0)
            return torch.empty((0, width), dtype=torch.float32, device=getattr(self.lm, "device", "cpu"))
        seqs = self._sequences(texts, prompt)
        pids, handle = self._prefix_handle(prompt) if prefixed and self._use_prefix(prompt) else ([], None)
        if handle is not None:
            # the tokens of prompt + text must BEGIN with the prompt's own tokens (a merge across the seam would change them)
            # and leave at least one token of the text's own: anything else takes the plain call
            k = len(pids)
            if all(len(s) > k and s[:k] == pids for s in seqs):
                seqs = [s[k:] for s in seqs]
            else:
                handle = None
        order = sorted(range(n), key=lambda i: -len(seqs[i]))         # longest first, like sentence-transformers
        lens = [len(seqs[i]) for i in order]
        parts, calls, padded = [], 0, 0
        for s, e in self._batches(lens):
            chunk = [seqs[i] for i in order[s:e]]
            parts.append(self._embed_prefixed(chunk, handle) if handle is not None else self._embed_plain(chunk))
            calls, padded = calls + 1, padded + (e - s) * (-(-lens[s] // 32) * 32)
        self.last_stats = dict(texts=n, lm_calls=calls, tokens=int(sum(lens)), padded_tokens=padded,
                               prefix_tokens=len(pids) if handle is not None else 0)
        cat = parts[0] if len(parts) == 1 else torch.cat(parts)
        if n == 1:
            return cat
        out = torch.empty_like(cat)
        out.index_copy_(0, torch.as_tensor(order, dtype=torch.int64, device=cat.device), cat)
        return out

    def _query_prompt(self) -> str:
        return self.prompt if self.query_prompt is None else self.query_prompt

    # -- the provider surface (HipBertEmbeddings') ---------------------------------------------------------------------
    def embed_documents_device(self, texts: List[str]):
        """Same embeddings as embed_documents, left on the device as one fp32 tensor [n][dim] (a device-resident store
        ingests them without the python-list round trip)."""
        return self._embed_device(list(texts), self.prompt, prefixed=False)

    def embed_queries_device(self, texts: List[str]):
        return self._embed_device(list(texts), self._query_prompt(), prefixed=True)

    def embed_documents(self, texts: List[str]) -> List[List[float]]:
        return self.embed_documents_device(texts).cpu().numpy().tolist() if texts else []

    def embed_queries(self, texts: List[str]) -> List[List[float]]:
        return self.embed_queries_device(texts).cpu().numpy().tolist() if texts else []

    def embed_query(self, text: str) -> List[float]:
        return self.embed_queries([text])[0]
