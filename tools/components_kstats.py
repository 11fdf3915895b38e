"""The rounds of one connected-components labelling kernel by kernel, from the kernel trace of

  rocprofv3 --kernel-trace --output-format csv -d D -- python3 tools/components_bench.py --trace
  python3 tools/components_kstats.py D [--label NAME]

Takes the LAST labelling of the trace (from its cc_init_kernel on) and cuts it at every cc_jump_kernel: a round is the hook
launches in front of a jump (by degree class: 8 lanes, the middle class, the workgroup lists) and that jump.  Prints one JSON
object with the microseconds of each, per round, and of the finish's kernels together: kernel time only, no launch gaps."""
import argparse
import csv
import glob
import json
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    files = glob.glob(os.path.join(args.trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        raise SystemExit(f"expected one *kernel_trace.csv under {args.trace_dir}, found {len(files)}")
    rows = []
    with open(files[0], newline="") as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"]
            if "cc_" in name:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if "cc_init_kernel" in r[2]]
    if not starts:
        raise SystemExit("no cc_init_kernel in this trace")
    run = rows[starts[-1] + 1:]
    rounds, cur, finish = [], {}, 0.0
    for t0, t1, name in run:
        us = (t1 - t0) / 1e3
        if "cc_jump_kernel" in name:
            cur["jump_us"] = round(us, 1)
            cur["hook_us"] = round(sum(v for k, v in cur.items() if k.startswith("hook_")), 1)
            rounds.append(cur)
            cur = {}
        elif "cc_hook_group_kernel" in name:
            key = "hook_8_lanes_us" if "ELi0E" in name or ", 0>" in name else "hook_middle_class_us"
            cur[key] = round(cur.get(key, 0.0) + us, 1)
        elif "cc_hook_block_kernel" in name:
            cur["hook_workgroup_us"] = round(cur.get("hook_workgroup_us", 0.0) + us, 1)
        else:
            finish += us
    out = {"label": args.label, "rounds": rounds, "finish_us": round(finish, 1),
           "hook_us_total": round(sum(r["hook_us"] for r in rounds), 1), "jump_us_total": round(sum(r["jump_us"] for r in rounds), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
