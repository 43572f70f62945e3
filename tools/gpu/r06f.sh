#!/bin/bash
# round 6: the whole GPU suite and smoke on the current tree, then the driver's bench command with its
# detail line kept, and the rocprofv3 kernel trace of the same command
cd "$GRAFT_REPO_ROOT" || exit 1
OUT=${OUT:-bench_out}                      # where this script keeps its logs and results
mkdir -p $OUT
export TMPDIR=/tmp
T=${TAG:-r06f}
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/${T}_pytest_gpu.txt 2>&1 || { tail -40 $OUT/${T}_pytest_gpu.txt; exit 1; }
tail -3 $OUT/${T}_pytest_gpu.txt
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${T}_smoke.txt 2>&1 || { cat $OUT/${T}_smoke.txt; exit 1; }
cat $OUT/${T}_smoke.txt
timeout -k 10 900 python3 bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${T}_bench.out 2> $OUT/${T}_bench.err || { tail -30 $OUT/${T}_bench.err; exit 1; }
tail -c 3000 $OUT/${T}_bench.out
