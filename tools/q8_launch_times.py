"""Per-launch times of rarc_scan_q8_kernel from a rocprofv3 --kernel-trace CSV: the launches of a cascaded scan repeat with a
fixed period (four per headline scan), so launch i of every scan is column i.  Prints median / min / max in us per position.
  python3 tools/q8_launch_times.py <kernel_trace.csv> [launches per scan = 4] [scans to skip = 5]"""
import csv
import statistics
import sys


def main():
    per = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    skip = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rows = [r for r in csv.DictReader(open(sys.argv[1])) if "rarc_scan_q8_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    scans = [us[i:i + per] for i in range(0, len(us) - per + 1, per)][skip:]
    print(f"{len(rows)} scan_q8 launches, {len(scans)} scans of {per} after {skip} skipped; us per launch position: median (min - max)")
    for i in range(per):
        col = [s[i] for s in scans]
        print(f"  launch {i + 1}: {statistics.median(col):9.1f} ({min(col):.1f} - {max(col):.1f})")
    tot = [sum(s) for s in scans]
    print(f"  scan    : {statistics.median(tot):9.1f} ({min(tot):.1f} - {max(tot):.1f})")


if __name__ == "__main__":
    main()
