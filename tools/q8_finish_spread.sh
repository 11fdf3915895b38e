#!/bin/bash
# How far apart do the persistent workgroups of a scan_q8 launch finish?  (the launch ends with its slowest workgroup,
# four times per cascaded scan.)  Measurement build of scan_q8 (-DRARC_EXPERIMENT -DRARC_Q8_ABLATIONS: the full kernel, plus a
# start and an end stamp per workgroup) behind tools/gpu_scan_only.py, RARC_Q8_FINISH naming the file the launcher appends to.
#   tools/q8_finish_spread.sh [rows] [dim] [f16|f8|shadow] [processes]      default: 100M x 768 fp16 rows, three fresh processes
# Prints every launch of the timed scans and the gate of the dynamic tail (tools/q8_finish_spread.py).
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R" || exit 1
V=rag-arc_amd/lib/librarc_var_abl.so
if [ ! -f $V ] || [ rag-arc_amd/csrc/scan_q8.hip -nt $V ] || [ rag-arc_amd/csrc/rarc_common.h -nt $V ]; then
  tools/build_variant_any.sh scan_q8 abl -DRARC_EXPERIMENT -DRARC_Q8_ABLATIONS || exit 1
fi
export RARC_LIBRARY=$R/$V RARC_ALLOW_EXPERIMENT=1
export PROBE_ROWS=${1:-100000000} PROBE_DIM=${2:-768} PROBE_ITERS=3; fmt=${3:-f16}; procs=${4:-3}
case $fmt in shadow) export PROBE_STORAGE=f16 PROBE_SHADOW=1;; *) export PROBE_STORAGE=$fmt;; esac
O=${Q8_FINISH_OUT:-$R/bench_outputs/q8_finish}; mkdir -p "$O"
ms=""; files=""
# every GPU process under its own time limit; the first one that fails (or prints no SCAN line) ends the script, its stderr is kept
for i in $(seq $procs); do
  rm -f "$O/finish_$i.txt"
  RARC_Q8_FINISH="$O/finish_$i.txt" timeout -k 10 420 python3 tools/gpu_scan_only.py > "$O/scan_$i.log" 2> "$O/scan_$i.log.err"; rc=$?
  if [ $rc -ne 0 ] || ! grep -q 'ms per scan' "$O/scan_$i.log" || [ ! -s "$O/finish_$i.txt" ]; then
    echo "process $i: exit status $rc"; tail -20 "$O/scan_$i.log.err"; exit 1
  fi
  ms="$ms${ms:+,}$(grep -o '[0-9.]* ms per scan' "$O/scan_$i.log" | cut -d' ' -f1)"; files="$files $O/finish_$i.txt"
done
echo "# tools/q8_finish_spread.sh $PROBE_ROWS $PROBE_DIM $fmt $procs: finishing times of the persistent workgroups of every scan_q8 launch"
echo "# (100 MHz clock, us; each process: one warm-up scan, then $PROBE_ITERS scans; the launcher waits for each launch, so the scan time"
echo "#  here includes four host round trips the product does not have)"
python3 tools/q8_finish_spread.py "$ms" $files
