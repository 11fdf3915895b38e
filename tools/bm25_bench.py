"""BM25 top-k on the MI355X: one JSON line.

A seeded Zipf corpus built through Bm25Index.from_token_ids (N documents of about --mean-len tokens over a 2^20 vocabulary),
--batch queries of --query-len tokens from the same law, k = --k.  Reports the batch rate of Bm25Device.topk (query upload,
the three kernels, answer download; device-synchronised), the posting bytes the batch touches (12 per posting: doc id +
fp64 weight) over the batch's kernel time as a fraction of the nominal 8 TB/s and of the read ceiling rarc_stream_read
measures, the host index build time, and the same restatement on host numpy (Bm25Index.host_scores + topk_order) as the
CPU comparison.  Kernel time comes from a separate `rocprofv3 --kernel-trace --stats` run of this tool (--trace-run: the
timed loop only), whose kernel_stats.csv is passed back with --kernel-stats.

  rocprofv3 --kernel-trace --stats -d OUT -o bm25 -- python tools/bm25_bench.py --trace-run
  python tools/bm25_bench.py --kernel-stats OUT/.../bm25_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0


def stream_read_GBps(torch, B, lib, dev, n_bytes=4 << 30):
    buf = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    buf.zero_()
    sink = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev)
    best = None
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        B.check(lib.rarc_stream_read(buf.data_ptr(), n_bytes, sink.data_ptr(), st.cuda_stream), "rarc_stream_read")
        b.record(st)
        b.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    del buf
    torch.cuda.empty_cache()
    return n_bytes / (best * 1e-3) / 1e9


def kernel_stats(path):
    """{kernel name: (calls, total ns)} of the rarc_bm25 kernels in a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            if "rarc_bm25" in name:
                short = name.split("(")[0].replace("void ", "")
                c, t = out.get(short, (0, 0))
                out[short] = (c + int(row["Calls"]), t + int(float(row["TotalDurationNs"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--mean-len", type=int, default=128)
    ap.add_argument("--vocab", type=int, default=1 << 20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--query-len", type=int, default=8)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-queries", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace-run", action="store_true", help="build, warm up and run the timed loop only (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a --trace-run under rocprofv3")
    a = ap.parse_args()

    import torch

    from rag_arc_amd.hip import binding as B
    from rag_arc_amd.hip.bm25 import Bm25Device, Bm25Index, synthetic_zipf, topk_order, zipf_terms

    if not torch.cuda.is_available():
        raise SystemExit("bm25_bench: no GPU (this tool measures the MI355X; nothing is timed on the CPU)")
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    off, ids = synthetic_zipf(a.docs, a.mean_len, a.vocab, seed=a.seed)
    t1 = time.perf_counter()
    idx = Bm25Index.from_token_ids(off, ids, n_terms=a.vocab)
    t2 = time.perf_counter()
    del ids
    gpu = Bm25Device(idx, device=0)
    t3 = time.perf_counter()
    rng = np.random.default_rng(a.seed + 1)
    queries = [idx.known_ids(zipf_terms(rng, a.query_len, a.vocab)) for _ in range(a.batch)]
    lens = idx.post_off[1:] - idx.post_off[:-1]
    postings = int(sum(int(lens[t]) for q in queries for t in q))
    bytes_batch = postings * 12

    for _ in range(a.warmup):
        gpu.topk(queries, a.k)
    torch.cuda.synchronize(dev)
    s = time.perf_counter()
    for _ in range(a.iters):
        got_i, got_s = gpu.topk(queries, a.k)
    torch.cuda.synchronize(dev)
    per_batch = (time.perf_counter() - s) / a.iters
    if a.trace_run:
        print(json.dumps({"trace_run": True, "batch_ms": round(per_batch * 1e3, 3)}))
        return

    # host numpy restatement: the same answers, timed on a few queries
    nh = min(a.host_queries, a.batch)
    s = time.perf_counter()
    for q in range(nh):
        sc = idx.host_scores(queries[q])
        want = topk_order(sc, a.k)
        assert np.array_equal(got_i[q], want) and np.array_equal(got_s[q].view(np.uint64), sc[want].view(np.uint64)), q
    host_qps = nh / (time.perf_counter() - s)

    out = {"what": "bm25_topk", "docs": a.docs, "mean_len": a.mean_len, "vocab": a.vocab, "batch": a.batch,
           "query_len": a.query_len, "k": a.k, "postings_total": int(idx.post_doc.size),
           "postings_per_batch": postings, "bytes_per_batch": bytes_batch,
           "qps": round(a.batch / per_batch, 1), "batch_ms": round(per_batch * 1e3, 3),
           "build_s": {"corpus": round(t1 - t0, 2), "index": round(t2 - t1, 2), "upload": round(t3 - t2, 2)},
           "host_numpy_qps": round(host_qps, 2), "host_checked_queries": nh}
    ceiling = stream_read_GBps(torch, B, B.load_library(), dev)
    out["stream_read_GBps"] = round(ceiling, 1)
    if a.kernel_stats:
        ks = kernel_stats(a.kernel_stats)
        calls = sum(c for n, (c, _) in ks.items() if "tile_kernel" in n)   # batches traced: one tile launch each
        kern_ns = sum(t for _, t in ks.values()) / calls
        out["kernels_us_per_batch"] = {n: round(t / calls / 1e3, 1) for n, (c, t) in ks.items()}
        out["kernel_us_per_batch"] = round(kern_ns / 1e3, 1)
        gbps = bytes_batch / kern_ns
        out["posting_GBps"] = round(gbps, 1)
        out["frac_of_8TBps"] = round(gbps / HBM_PEAK_GBS, 4)
        out["frac_of_stream_read"] = round(gbps / ceiling, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
