#!/usr/bin/env python3
"""Decoder-LM embeddings on the GPU, timed next to the reranker step they share a forward with (DESIGN, "Decoder-LM
embeddings").  GPU only, one process; every step runs under its own time limit (SIGALRM: a step that overruns ends the process —
nothing more is started behind a hang).

Qwen3-Embedding-0.6B geometry (28 layers, hidden 1024, 16 query / 8 K/V heads of 128, ffn 3072), seeded weights, a reduced
vocabulary (the embedding table is a gather: its size does not enter the timings):
  1. documents per second: embed_last_device on batches of 128- and 512-token documents (`--batch-tokens` padded tokens per
     call), and yes_no_logits_device on the same batches — the same forward up to its last kernel;
  2. embed_query p50 (host clock: text in, python floats out) for a 17-token query prompt and 6- to 12-token queries, with the
     prefix cache and without it; and the plain LM calls at the same token counts: embed_last and yes_no_logits on the 4 x 32 /
     4 x 64 token batches those queries make (device result copied to the host).
Each timing: `--warmup` unmeasured calls, then `--repeats` measured ones; the JSON carries min / median / max.

    python3 tools/lm_embed_bench.py --out profiles/lm_embed_bench.json
"""
import argparse
import json
import os
import re
import signal
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class StepTimeout(Exception):
    pass


def _alarm(signum, frame):
    raise StepTimeout()


def step(name, limit_s, fn):
    """fn() under a time limit of its own; an overrun or an error ends the process."""
    signal.signal(signal.SIGALRM, _alarm)
    signal.alarm(int(limit_s))
    try:
        return fn()
    except StepTimeout:
        print(f"lm_embed_bench: step '{name}' exceeded {limit_s} s: stopping", file=sys.stderr, flush=True)
        os._exit(124)
    finally:
        signal.alarm(0)


def timed(torch, fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return {"min_s": min(out), "median_s": statistics.median(out), "max_s": max(out), "repeats": len(out)}


def seeded_state_dict(torch, H, LAYERS, NQ, NKV, DH, I, V, seed):
    """oracle.random_qwen3_state_dict's distributions, drawn on the device (0.6 G parameters)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g, device="cuda") * 0.05
    sd = {"model.embed_tokens.weight": r(V, H) * 4, "model.norm.weight": 1 + r(H)}
    for i in range(LAYERS):
        p = f"model.layers.{i}."
        sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"] = r(NQ * DH, H), r(NKV * DH, H)
        sd[p + "self_attn.v_proj.weight"], sd[p + "self_attn.o_proj.weight"] = r(NKV * DH, H), r(H, NQ * DH)
        sd[p + "self_attn.q_norm.weight"], sd[p + "self_attn.k_norm.weight"] = 1 + r(DH), 1 + r(DH)
        sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"], sd[p + "mlp.down_proj.weight"] = r(I, H), r(I, H), r(H, I)
        sd[p + "input_layernorm.weight"], sd[p + "post_attention_layernorm.weight"] = 1 + r(H), 1 + r(H)
    return sd


WORD = re.compile(r"\w+|[^\w\s]")
QUERY_PROMPT = "Instruct: Given a web search query, retrieve relevant passages that answer the query\nQuery:"
QUERIES = ["what is a vector index", "how does cosine similarity differ from the inner product",
           "which GPUs have 288 GB of memory", "when should a reranker follow the dense retriever in a pipeline",
           "exact top-k search versus approximate nearest neighbours", "why are decoder embedders left padded",
           "what does Matryoshka truncation do to an embedding", "how many tokens fit into one batch"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--doc-tokens", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--batch-tokens", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--vocab", type=int, default=32768)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--query-repeats", type=int, default=50)
    ap.add_argument("--limit", type=int, default=120, help="seconds per step")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("lm_embed_bench: no ROCm device visible (this tool measures on the GPU only)")
    from rag_arc_amd.core.rerank import HipCausalLM
    from rag_arc_amd.encapsulation.embeddings.hip_qwen3 import HipQwen3Embeddings

    H, NQ, NKV, DH, I, V = 1024, 16, 8, 128, 3072, a.vocab
    lm = step("weights", a.limit, lambda: HipCausalLM(seeded_state_dict(torch, H, a.layers, NQ, NKV, DH, I, V, 6), NQ, NKV, DH))
    dev = lm.device
    result = {"device": torch.cuda.get_device_name(0), "geometry": dict(hidden=H, layers=a.layers, n_q=NQ, n_kv=NKV, head_dim=DH, ffn=I, vocab=V),
              "warmup": a.warmup, "repeats": a.repeats, "batch_tokens": a.batch_tokens, "documents": [], "queries": {}}
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    for L in a.doc_tokens:
        n = max(4, a.batch_tokens // L)
        ids = torch.randint(5, V, (n, L), generator=g, device="cuda", dtype=torch.int32)
        start = torch.zeros(n, dtype=torch.int32, device=dev)
        rec = {"doc_tokens": L, "docs_per_call": n}
        rec["embed_last"] = step(f"embed {L}", a.limit, lambda: timed(torch, lambda: lm.embed_last_device(ids, start), a.warmup, a.repeats))
        rec["yes_no_logits"] = step(f"logits {L}", a.limit,
                                    lambda: timed(torch, lambda: lm.yes_no_logits_device(ids, start, 11, 42), a.warmup, a.repeats))
        for k in ("embed_last", "yes_no_logits"):
            rec[k]["docs_per_s"] = n / rec[k]["median_s"]
            rec[k]["tokens_per_s"] = n * L / rec[k]["median_s"]
        rec["embed_over_logits"] = rec["embed_last"]["median_s"] / rec["yes_no_logits"]["median_s"]
        result["documents"].append(rec)
        print(json.dumps(rec), flush=True)

    tok = lambda text: [5 + hash_word(w) % (V - 5) for w in WORD.findall(text)]
    n_prompt = len(tok(QUERY_PROMPT))
    q = {"prompt_tokens": n_prompt, "query_tokens": [len(tok(t)) for t in QUERIES]}
    for key, cache in (("embed_query_prefix_cache", True), ("embed_query_plain", False)):
        emb = HipQwen3Embeddings(lm, tok, query_prompt=QUERY_PROMPT, eos_token_id=4, prefix_cache=cache)
        it = iter(range(1 << 30))
        q[key] = step(key, a.limit, lambda: timed(torch, lambda: emb.embed_query(QUERIES[next(it) % len(QUERIES)]), a.warmup, a.query_repeats))
        q[key]["last_stats"] = {k: int(v) for k, v in emb.last_stats.items()}
    q["prefix_over_plain"] = q["embed_query_prefix_cache"]["median_s"] / q["embed_query_plain"]["median_s"]
    for L in (32, 64):                                    # the batches one such query makes: 4 rows, one real
        ids = np.zeros((1, L), np.int32)
        ids[0] = np.arange(5, 5 + L)
        mask = np.ones((1, L), np.int8)
        q[f"embed_last_4x{L}"] = step(f"embed 4x{L}", a.limit, lambda: timed(torch, lambda: lm.embed_last(ids, mask).cpu(), a.warmup, a.query_repeats))
        q[f"yes_no_logits_4x{L}"] = step(f"logits 4x{L}", a.limit,
                                         lambda: timed(torch, lambda: lm.yes_no_logits(ids, mask, 11, 42).cpu(), a.warmup, a.query_repeats))
    result["queries"] = q
    print(json.dumps(q), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps({"lm_embed_bench": "done"}))


def hash_word(w):
    """A stable id per word (python's hash() is salted per process)."""
    h = 2166136261
    for b in w.encode("utf-8"):
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


if __name__ == "__main__":
    main()
