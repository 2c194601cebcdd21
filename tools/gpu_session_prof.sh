#!/bin/bash
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-session_out}
mkdir -p "$OUT"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_bench3 -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-secondary > "$OUT"/prof_bench3.log 2>&1
tail -1 "$OUT"/prof_bench3.log | cut -c1-300
