#!/bin/bash
# round-6 evidence on the committed tree: GPU suite + smoke, the driver's bench command (timed),
# the same command under rocprofv3 --kernel-trace --stats, separate PMC passes on the C2 line, and
# the FETCH/WRITE calibration of the QT launch's access patterns (tools/fetch_calib.hip).
#   bash tools/gpu/r06_evidence.sh TAG     (outputs $OUT/<TAG>_*)
# (the large-N counters are a call of their own: tools/gpu/r06_large_pmc.sh)
TAG=${1:-r06}
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}                      # where this script keeps its logs and results
mkdir -p $OUT
export TMPDIR=/tmp
R="$GRAFT_REPO_ROOT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q -rP --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?
grep -E "^C[345]|^1M|^world|^C2 headline|^MD step|passed|failed|Error|^E " $OUT/pytest_gpu.log | head -60
[ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { cat $OUT/smoke.log; exit 1; }
tail -1 $OUT/smoke.log
start=$(date +%s)
timeout -k 10 900 python3 -u bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/bench_full.log 2> $OUT/bench_full.err || { tail -30 $OUT/bench_full.err; exit 1; }
echo "bench wall $(( $(date +%s) - start )) s"
tail -1 $OUT/bench_full.log > $OUT/${TAG}_full_bench.json
grep "^BENCH_DETAIL " $OUT/bench_full.err | sed 's/^BENCH_DETAIL //' > $OUT/${TAG}_bench_detail.json
wc -c $OUT/${TAG}_full_bench.json
cd /tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$R/$OUT/prof_$TAG" -o run -- python3 "$R/bench.py" --full --gpus 1 --steps 20 --warmup 5 > "$R/$OUT/prof_$TAG.log" 2>&1 || { tail -5 "$R/$OUT/prof_$TAG.log"; exit 1; }
B="$R/bench.py --steps 20 --warmup 5 --no-cpu-baseline --sharded-config none --million-config none --no-pump-lines --no-mcmd-lines --md-only-config none --no-e2e-line --no-replicas-line"
timeout -s KILL 90 rocprofv3 --pmc FETCH_SIZE -d "$R/$OUT/pmc_fetch" -o run -- python3 $B > "$R/$OUT/pmc_fetch.log" 2>&1 || exit $?
timeout -s KILL 90 rocprofv3 --pmc WRITE_SIZE -d "$R/$OUT/pmc_write" -o run -- python3 $B > "$R/$OUT/pmc_write.log" 2>&1 || exit $?
timeout -s KILL 90 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_SALU SQ_INSTS_LDS GRBM_GUI_ACTIVE -d "$R/$OUT/pmc_sq" -o run -- python3 $B > "$R/$OUT/pmc_sq.log" 2>&1 || exit $?
timeout -s KILL 60 rocprofv3 --pmc FETCH_SIZE -d "$R/$OUT/cal_fetch" -o run -- "$R/tools/fetch_calib" > "$R/$OUT/cal_fetch.log" 2>&1 || exit $?
timeout -s KILL 60 rocprofv3 --pmc WRITE_SIZE -d "$R/$OUT/cal_write" -o run -- "$R/tools/fetch_calib" > "$R/$OUT/cal_write.log" 2>&1 || exit $?
cd "$R"
db() { ls $OUT/$1/*/*.db $OUT/$1/*.db 2>/dev/null | head -1; }
python3 tools/prof_summary.py $(db prof_$TAG) > $OUT/${TAG}_driver_cmd_kernel_stats.txt
python3 tools/prof_mainline.py $(db prof_$TAG) 24 > $OUT/${TAG}_driver_cmd_headline_kernels.txt 2>&1 || true
python3 tools/pmc_summary.py $(db cal_fetch) $(db cal_write) > $OUT/${TAG}_fetch_calib.json
cat $OUT/cal_fetch.log | grep "known bytes" > $OUT/${TAG}_fetch_calib_known.txt
FACT=$(python3 tools/calib_factors.py $OUT/${TAG}_fetch_calib.json $OUT/${TAG}_fetch_calib_known.txt)
echo "calibration factors (fetch write): $FACT"
python3 tools/pmc_summary.py $(db pmc_fetch) $(db pmc_write) $(db pmc_sq) --factors $FACT > $OUT/${TAG}_c2_pmc.json
grep "^{" $OUT/prof_$TAG.log | tail -1 > $OUT/${TAG}_driver_cmd_bench_under_rocprof.json || true
head -12 $OUT/${TAG}_driver_cmd_kernel_stats.txt
head -12 $OUT/${TAG}_driver_cmd_headline_kernels.txt
python3 tools/bench_brief.py $OUT/${TAG}_full_bench.json
