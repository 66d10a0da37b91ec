#!/bin/bash
# rocprofv3 kernel trace of a short bench run (GPU box): per-kernel summary -> $OUT/prof_summary.md
R="${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}"
OUT="${OUT:-$R/bench_out}"
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp
ARGS="${BENCH_ARGS:---full --tokens 32 --steps 1 --warmup 1 --cpu-baseline 0}"
timeout -k 10 ${T_PROF:-600} rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 "$R/bench.py" $ARGS > "$OUT/prof.log" 2>&1
rc=$?; echo "rocprof rc=$rc"; tail -3 "$OUT/prof.log"
[ $rc -eq 0 ] || exit $rc
python3 "$R/tools/prof_summary.py" "$OUT/prof" "$OUT/prof_summary.md" | head -40
