#!/bin/bash
# Kernel trace of config 5 steps (gaps between launches).
set -o pipefail
R=${GRAFT_REPO_ROOT:-/root/repo}
OUT=$R/gpurun_out/${TAG:-c5trace}; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --output-format csv -d $OUT/kt -o kt -- python3 $R/bench.py --workload config5 --steps 10 --warmup 2 --full --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err
