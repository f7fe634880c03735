#!/bin/bash
# Device time of a SLAM chunk with a given feat_rep_slam (for information: a single inverse depth landmark is two
# covariance rows smaller than a three-parameter one).  One rocprofv3 kernel trace of the bench workload per
# representation, summarized by tools/slam_chunk_time.py and tools/prof_summary.py.
# usage: bash tools/gpu_rep_chunk.sh OUTDIR [WORKLOAD] [REP ...]      (defaults: cfg3, representations 4 and 5)
set -e -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=$1; WL=${2:-cfg3}; shift || true; shift || true
REPS=${*:-4 5}
mkdir -p "$O"
O=$(cd "$O" && pwd)
export TMPDIR=/tmp
for rep in $REPS; do
  (cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$O/rep$rep" -o run -- \
     python3 "$R/bench.py" --workload "$WL" --steps 200 --cpu-frames 0 --set feat_rep_slam=$rep \
     > "$O/rep$rep.json" 2> "$O/rep$rep.err")
  python3 "$R/tools/slam_chunk_time.py" "$O/rep$rep/run_kernel_trace.csv" > "$O/rep${rep}_slam_chunk.txt"
  python3 "$R/tools/prof_summary.py" "$O/rep$rep/run_kernel_trace.csv" > "$O/rep${rep}_per_frame.txt"
  rm -rf "$O/rep$rep"
done
