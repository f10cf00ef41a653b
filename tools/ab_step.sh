#!/bin/bash
# whole-step times (HIP events around 20 executes, tools/probes/p1_probe.py) of several builds of the library, alternating:
#   bash tools/ab_step.sh "prev amd" cfg3_gaussian2_xy [more configs]      REPS=5 by default
# a config may carry p1_probe.py's further arguments: "cfg3_gaussian2_xy 512x512 tiled", "cfg3_gaussian2_xy 16384x16380"
# (the first process that fails ends the run)
set -o pipefail
root=$(pwd)
libs=$1; shift
REPS=${REPS:-5}
for c in "$@"; do for rep in $(seq $REPS); do for v in $libs; do
  export RECFILTER_AMD_LIB=$root/recfilter_amd/librecfilter_$v.so
  timeout -k 10 120 python3 $root/tools/probes/p1_probe.py $c 2>/dev/null | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); print('$v $c step_ms', d['step_ms'], ' '.join(f'{k}={v}' for k,v in d['kernels'].items()))" || { echo "$v $c: failed"; exit 1; }
done; done; done
