"""Metric "l2" next to its baseline: ms per 256-query batch of rarc_search_wide_l2 and of rarc_search_wide (metric "ip", the
same rows, the same queries, the same process) at k = 100 on fp16 rows — both through FlatIndexF16._search_wide_chunk, i.e. with
query prep, the status read-back and the capacity protocol.  The L2 search adds one 4-byte load per row and tile and a few
VALU operations per nominee.

    python tools/l2_bench.py --rows 1000000,10000000 --dim 768 --out profiles/l2_bench.json

Prints one JSON line per size (and writes them all to --out): per-batch times in rounds of `--reps` batches — median round,
fastest, slowest — for both metrics, the ratio of the medians, each metric's own round-to-round spread, and the time and
rate of rarc_row_sqnorms over all rows (median of five calls, each synchronised on both sides)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from rag_arc_amd.hip import binding as B  # noqa: E402
from rag_arc_amd.hip.engine import FlatIndexF16  # noqa: E402


def rounds(idx, q, k, reps, n_rounds):
    out_ids = torch.empty((q.shape[0], k), dtype=torch.int64, device=q.device)
    out_sc = torch.empty((q.shape[0], k), dtype=torch.float32, device=q.device)
    ms = []
    with idx._lock, torch.cuda.device(q.device):
        for _ in range(3):
            idx._search_wide_chunk(q, k, out_ids, out_sc)
        for _ in range(n_rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                idx._search_wide_chunk(q, k, out_ids, out_sc)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / reps * 1e3)
    return sorted(ms), out_ids.clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib, dev = B.load_library(), torch.device("cuda", 0)
    d, d_pad = a.dim, B.padded_dim(a.dim)
    q = torch.empty((a.queries, d), dtype=torch.float32, device=dev)
    B.check(lib.rarc_synth_rows_f32(q.data_ptr(), d, d, 0, a.queries, 4321, 0))
    results = []
    for n in [int(v) for v in a.rows.split(",")]:
        buf = torch.empty((n, d_pad), dtype=torch.float16, device=dev)
        B.check(lib.rarc_synth_rows_f16(buf.data_ptr(), d_pad, d, 0, n, 1234, 0))
        res = {"rows": n, "dim": d, "d_pad": d_pad, "k": a.k, "queries": a.queries, "storage": "f16", "reps_per_round": a.reps}
        for metric in ("ip", "l2", "ip", "l2"):                # interleaved: drift of the box shows up in both
            idx = FlatIndexF16(d, metric=metric, growable=False)
            idx.add_rows_f16(buf, 1.001)
            if metric == "l2":                                 # rarc_row_sqnorms over all rows, alone on the device
                times = []
                for _ in range(6):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    idx._update_xn(0)
                    torch.cuda.synchronize()
                    times.append((time.perf_counter() - t0) * 1e3)
                ms_n = sorted(times[1:])[len(times[1:]) // 2]      # (the first call is the warm-up)
                res["row_sqnorms_ms"] = round(ms_n, 4)
                res["row_sqnorms_tb_per_s"] = round(n * d_pad * 2 / (ms_n * 1e-3) / 1e12, 3)
            ms, _ = rounds(idx, q, a.k, a.reps, a.rounds)
            res.setdefault(metric + "_ms_rounds", []).extend(round(v, 4) for v in ms)
            res[metric + "_cap"] = int(idx.last_wide_cap)
            del idx
        for metric in ("ip", "l2"):
            v = sorted(res[metric + "_ms_rounds"])
            res[metric + "_ms"] = v[len(v) // 2]
            res[metric + "_spread_pct"] = round((v[-1] - v[0]) / v[len(v) // 2] * 100, 2)
        res["l2_over_ip"] = round(res["l2_ms"] / res["ip_ms"], 4)
        res["gemm_bound_ms"] = round(2.0 * 256 * n * d_pad / 2.5e15 * 1e3, 4)        # MFMA fp16 dense peak, 2.5 PF
        print(json.dumps(res), flush=True)
        results.append(res)
        del buf
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
