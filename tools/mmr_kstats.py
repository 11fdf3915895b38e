"""The batched MMR call kernel by kernel, from the `*kernel_stats.csv` of ONE cell's trace:

  rocprofv3 --kernel-trace --stats --output-format csv -d D -- python tools/mmr_bench.py --batched-only --cells 5 20
  python tools/mmr_kstats.py D/<host>/<pid>_kernel_stats.csv --calls 10 --cell 5 20

`--calls` is the number of batched calls the traced run made (mmr_bench.py --batched-only: ten).  Prints one JSON object: GPU time
per batched call of rarc_mmr_rows_kernel, of the search's own kernels (every library kernel of the trace that runs once or
more per call: query prep, seed, scan, rescore, finalize — not the index build's ingest / quantisation kernels, not torch's),
and their ratio.  Both sides are kernel time from the same trace: no host time, no copies."""
import argparse
import csv
import json

BUILD = ("rarc_ingest", "rarc_quant_meta", "rarc_l2norm", "rarc_synth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stats_csv")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--cell", type=int, nargs=2, default=None, metavar=("K", "FETCH_K"))
    args = ap.parse_args()
    mmr_ns, search = 0.0, {}
    with open(args.stats_csv, newline="") as fh:
        for row in csv.DictReader(fh):
            name, total = row["Name"], float(row["TotalDurationNs"])
            short = name.split("(")[0].replace("void ", "")
            if "rarc_mmr_rows_kernel" in name:
                mmr_ns += total
            elif "rarc_" in name and not any(b in name for b in BUILD) and int(row["Calls"]) >= args.calls:
                search[short] = search.get(short, 0.0) + total
    if not mmr_ns:
        raise SystemExit("no rarc_mmr_rows_kernel in this trace")
    per = lambda ns: round(ns / args.calls / 1e6, 4)
    out = {"cell": args.cell, "batched_calls": args.calls, "mmr_rows_kernel_ms": per(mmr_ns),
           "search_kernels_ms": per(sum(search.values())), "search_kernels": {k: per(v) for k, v in sorted(search.items())}}
    out["mmr_over_search_kernels"] = round(out["mmr_rows_kernel_ms"] / out["search_kernels_ms"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
