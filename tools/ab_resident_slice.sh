#!/bin/bash
# A/B of the 16x16x32 trunk kernel's resident slice on one box, in one session.
#   tools/ab_resident_slice.sh <checkout of the parent commit, library built> [pairs]     parent / this tree, interleaved
#   tools/ab_resident_slice.sh - [pairs]                                                    this tree alone: NRNERF_RESIDENT_SLICE=0 / 1, interleaved
# One line per run: rays/s, ms per step, the kernels' ms per step.  Every GPU step has its own time limit and the script stops at the
# first step that fails: nothing is started on the device after a failure.
set -o pipefail
HERE="$(cd "$(dirname "$0")/.." && pwd)"
PARENT="${1:?a checkout of the parent commit with its library built, or - for the in-build switch}"
PAIRS="${2:-3}"
BENCH="python bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-psnr --no-train-step --min-gpu-seconds 0"
SHOW='import sys,json; d=json.loads(sys.stdin.read()); r=d["roofline"]; print(d["value"], d["ms_per_step"], json.dumps(r["kernels_ms_per_step"]))'
run() {      # label, directory, environment assignment
  echo -n "$1: "
  (cd "$2" && env $3 timeout -k 10 300 $BENCH 2>/dev/null | tail -1 | python -c "$SHOW") || { echo "FAILED: $1"; exit 1; }
}
for i in $(seq 1 "$PAIRS"); do
  if [ "$PARENT" = "-" ]; then
    run "pair $i resident_slice=0" "$HERE" NRNERF_RESIDENT_SLICE=0
    run "pair $i resident_slice=1" "$HERE" NRNERF_RESIDENT_SLICE=1
  else
    run "pair $i parent" "$PARENT" NRNERF_RESIDENT_SLICE=1
    run "pair $i change" "$HERE" NRNERF_RESIDENT_SLICE=1
  fi
done
