#!/bin/bash
# kernel trace of the end-to-end line (mdqt_run at the reference cadence) only
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}                      # where this script keeps its logs and results
mkdir -p $OUT
export TMPDIR=/tmp
R="$GRAFT_REPO_ROOT"
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --stats -d "$R/$OUT/prof_e2e" -o run -- python3 "$R/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline --sharded-config none --million-config none --no-pump-lines --no-mcmd-lines --md-only-config none --no-replicas-line > "$R/$OUT/prof_e2e.log" 2>&1 || { tail -5 "$R/$OUT/prof_e2e.log"; exit 1; }
cd "$R"
python3 tools/prof_summary.py $(ls $OUT/prof_e2e/*/*.db $OUT/prof_e2e/*.db 2>/dev/null | head -1) | head -25
