#!/bin/bash
# Developer aid (GPU box): sample the shader clock / power while rowgemm_bench.py loops.  Usage: tools/clock_probe.sh
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
REPS=${REPS:-6000} python $ROOT/tools/rowgemm_bench.py 2>/dev/null &
pid=$!
sleep ${WARM:-14}
for i in 1 2 3; do
  rocm-smi --showclocks --showpower 2>/dev/null | grep -E "sclk|Power" | tr -s ' ' | head -4
  sleep 0.3
done
wait $pid
