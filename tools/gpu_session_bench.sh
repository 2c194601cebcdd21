#!/bin/bash
# One GPU session: headline bench, kernel-trace profile of the same command, PMC traffic passes for the
# dominant elementwise kernel.  Outputs land in $OUT (default session_out/) and are copied into profiles/ by tools/collect_profiles.py
# (run with the same OUT).
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-session_out}
mkdir -p "$OUT"
python bench.py --steps 5 --warmup 2 --full > "$OUT"/bench_n1.json 2> "$OUT"/bench_n1.err
cat "$OUT"/bench_n1.json
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_bench -- python3 bench.py --steps 5 --warmup 2 --full --no-cpu-baseline --no-secondary > "$OUT"/prof_bench.log 2>&1
python tools/window_breakdown.py "$OUT"/prof_bench --windows 5 > "$OUT"/window_breakdown.txt 2>&1
cat "$OUT"/window_breakdown.txt | head -40
if [ "$1" != "quick" ]; then
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/prof_roofline -- python3 tools/roofline_only.py > "$OUT"/prof_roofline.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT"/pmc_fetch -- python3 tools/roofline_only.py > "$OUT"/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT"/pmc_write -- python3 tools/roofline_only.py > "$OUT"/pmc_write.log 2>&1
fi
# the raw traces are large: keep the summaries only
find "$OUT"/prof_bench -name "*kernel_trace.csv" -delete
find "$OUT" -name "*stats.csv" -newer "$OUT"/bench_n1.json | head
