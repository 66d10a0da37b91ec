#!/bin/bash
# GPU box: full default bench (with the CPU baseline leg), then a rocprofv3 kernel-trace summary of
# the same command (CPU leg off). Every GPU step has its own time limit; a failure ends the run.
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT="${OUT:-$R/bench_out}"
cd "$R" && mkdir -p "$OUT"
timeout -k 10 900 python bench.py --full ${BENCH_ARGS} > $OUT/bench.log 2> $OUT/bench.err
rc=$?; echo "bench rc=$rc"; tail -3 $OUT/bench.err; cat $OUT/bench.log
[ $rc -eq 0 ] || exit $rc
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 "$R/bench.py" --full ${BENCH_ARGS} --cpu-baseline 0 > "$OUT/prof.log" 2>&1
rc=$?; echo "rocprof rc=$rc"; tail -2 "$OUT/prof.log"
[ $rc -eq 0 ] || exit $rc
python3 "$R/tools/prof_summary.py" "$OUT/prof" "$OUT/prof_summary.md" | head -30
