#!/bin/bash
# What the int8-prefilter scan's time is made of, at the bench's own size and thresholds: the ablated instantiations of a
# measurement build of scan_q8 (wrong results on purpose: -DRARC_EXPERIMENT -DRARC_Q8_ABLATIONS) behind tools/gpu_scan_only.py.
#   tools/q8_abl.sh [rows] [dim] [f16|f8|shadow] [rounds] [abl values...]
# default: 100M x 768 fp16 rows, two rounds of
#   0 full kernel | 262144 full kernel, plain row loads | 5 skeleton (no MFMAs, no pruning) | 262149 skeleton, plain row loads
# (the row stream's cache policy, A/B in one binary).  Other values: see ABL in rag-arc_amd/csrc/scan_q8.hip (1 no pruning,
# 4 no MFMAs, 9 ...).  What a tile's loads without row bytes cost:  tools/q8_abl.sh 100000000 768 f16 2 0 8 524288 524296
# (8 no threshold / histogram refresh, 524288 the tile's metadata pair a constant, 524296 both).
#   tools/q8_abl.sh clock [rows] [dim] [f16|f8|shadow] [abl values...]   the variants' shader clock instead (default: the four above): one own --pmc GRBM_GUI_ACTIVE pass
#                                        each (busy shader cycles per launch) over the launch time of the same run
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R" || exit 1
clock=0; if [ "${1:-}" = clock ]; then clock=1; shift; fi
# the measurement library must be built from THIS scan_q8.hip: an older one knows no 262144 and would run the full kernel under that name
V=rag-arc_amd/lib/librarc_var_abl.so
if [ ! -f $V ] || [ rag-arc_amd/csrc/scan_q8.hip -nt $V ] || [ rag-arc_amd/csrc/rarc_common.h -nt $V ]; then
  tools/build_variant_any.sh scan_q8 abl -DRARC_EXPERIMENT -DRARC_Q8_ABLATIONS || exit 1
fi
export RARC_LIBRARY=$R/$V RARC_ALLOW_EXPERIMENT=1
if [ $clock = 1 ]; then set -- "${1:-100000000}" "${2:-768}" "${3:-f16}" 1 "${@:4}"; fi   # (no rounds argument in clock mode)
export PROBE_ROWS=${1:-100000000} PROBE_DIM=${2:-768} PROBE_ITERS=3; fmt=${3:-f16}; rounds=${4:-2}; shift; shift; shift; shift
case $fmt in shadow) export PROBE_STORAGE=f16 PROBE_SHADOW=1;; *) export PROBE_STORAGE=$fmt;; esac
O=${Q8_ABL_OUT:-$R/bench_outputs/q8_abl}; mkdir -p "$O"   # logs, stderr and counter output of every run
# every GPU process under its own time limit; the first one that fails (or prints no SCAN line) ends the script, its stderr is kept
run() {  # run <abl> <log> <command...>
  abl=$1; log=$2; shift; shift
  RARC_Q8_ABL=$abl timeout -k 10 300 "$@" > "$log" 2> "$log.err"; rc=$?
  if [ $rc -ne 0 ] || ! grep -q SCAN "$log"; then echo "abl $abl: exit status $rc"; tail -20 "$log.err"; exit 1; fi
}
if [ $clock = 1 ]; then
  for abl in ${@:-0 262144 5 262149}; do
    rm -rf "$O/pmc_$abl"
    run $abl "$O/clock_$abl.log" rocprofv3 --pmc GRBM_GUI_ACTIVE -d "$O/pmc_$abl" -- python3 tools/gpu_scan_only.py
    ms=$(grep -o '[0-9.]* ms per scan' "$O/clock_$abl.log" | cut -d' ' -f1); n=$(grep -o '([0-9]* launches' "$O/clock_$abl.log" | tr -dc 0-9)
    cyc=$(python3 tools/pmc_summary.py "$O/pmc_$abl" | grep scan_q8 | grep GRBM_GUI_ACTIVE | sed 's/.*unrounded mean \([0-9.]*\).*/\1/' | head -1)
    python3 -c "import sys; ms, n, c = float(sys.argv[1]), int(sys.argv[2]), float(sys.argv[3]); print('abl %6s %s x %s %s: %.3f ms per launch, %.4e busy shader cycles per launch -> %.0f MHz' % (sys.argv[4], sys.argv[5], sys.argv[6], sys.argv[7], ms / n, c, c / (ms / n) / 1e3))" "$ms" "$n" "$cyc" $abl $PROBE_ROWS $PROBE_DIM $fmt || exit 1
    find "$O/pmc_$abl" -name "*.db" -delete 2>/dev/null
  done
  exit 0
fi
for r in $(seq $rounds); do
  for abl in ${@:-0 262144 5 262149}; do
    run $abl "$O/scan_$abl.log" python3 tools/gpu_scan_only.py
    grep SCAN "$O/scan_$abl.log"
  done
done
