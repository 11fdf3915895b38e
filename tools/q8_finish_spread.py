"""Summary of the files tools/q8_finish_spread.sh leaves (one line per scan_q8 launch, written by the measurement build under
RARC_Q8_FINISH): per process and scan, what the launches lose to workgroups that finish apart, and the gate of the dynamic
tail: the sum over a scan's launches of (last - median) finishing time against 0.5 % of the scan.
  python3 tools/q8_finish_spread.py <scan ms per process, comma separated> <file of process 1> <file of process 2> ..."""
import re
import sys

PAT = re.compile(r"launch tiles \[(\d+), (\d+)\) grid (\d+): ([\d.]+) us \| ends: last-first ([\d.]+) us .*? last-median ([\d.]+) us .*? "
                 r"last-mean ([\d.]+) us")


def scans_of(path):
    """The launches of a file, grouped into scans (a scan starts at tile 0); the first scan is the warm-up and is dropped."""
    scans = []
    for line in open(path):
        m = PAT.search(line)
        if not m:
            continue
        rec = dict(t0=int(m[1]), t1=int(m[2]), grid=int(m[3]), us=float(m[4]), lf=float(m[5]), lmed=float(m[6]), lmean=float(m[7]),
                   raw=line.rstrip())
        if rec["t0"] == 0:
            scans.append([])
        if scans:
            scans[-1].append(rec)
    return scans[1:]


def main():
    ms = [float(x) for x in sys.argv[1].split(",")]
    shares = []
    for i, path in enumerate(sys.argv[2:]):
        print(f"== process {i + 1}: {ms[i]:.3f} ms per scan (device events around the launches) ==")
        for j, scan in enumerate(scans_of(path)):
            for r in scan:
                print(r["raw"])
            tot = sum(r["us"] for r in scan)
            lmed, lmean, lf = (sum(r[k] for r in scan) for k in ("lmed", "lmean", "lf"))
            share = 100 * lmed / (ms[i] * 1e3)
            shares.append(share)
            print(f"scan {j + 1}: {len(scan)} launches, {tot:.1f} us inside them; summed over the launches: last-median {lmed:.1f} us = "
                  f"{share:.2f} % of the scan, last-mean {lmean:.1f} us = {100 * lmean / (ms[i] * 1e3):.2f} %, last-first {lf:.1f} us = "
                  f"{100 * lf / (ms[i] * 1e3):.2f} %")
    shares.sort()
    med = 0.5 * (shares[(len(shares) - 1) // 2] + shares[len(shares) // 2])
    print(f"gate: sum of (last - median) over a scan's launches, {len(shares)} scans: median {med:.2f} % of the scan (min {shares[0]:.2f} %, "
          f"max {shares[-1]:.2f} %); the dynamic tail is built at 0.5 % or more -> {'BUILD' if med >= 0.5 else 'STOP'}")


if __name__ == "__main__":
    main()
