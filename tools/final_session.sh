#!/bin/bash
# Round-end GPU session: the GPU test suite, smoke(), the driver's bench
# command, and a kernel trace (--kernel-trace --stats) of the same command.
# Every GPU step has its own time limit; the first failure ends the session.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp && OUT=${OUT:-bench_out} && mkdir -p "$OUT"
T=${TAG:-final}
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread \
  > $OUT/${T}_tests.log 2>&1 || { tail -30 $OUT/${T}_tests.log; exit 1; }
tail -2 $OUT/${T}_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${T}_smoke.log 2>&1 \
  || { tail -30 $OUT/${T}_smoke.log; exit 1; }
tail -1 $OUT/${T}_smoke.log
timeout -k 10 400 python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --secondary-out $OUT/${T}_bench_secondary.json \
  > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err || { tail -30 $OUT/${T}_bench.err; exit 1; }
tail -c 600 $OUT/${T}_bench.json
rm -rf $OUT/${T}_prof
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/${T}_prof -o run --output-format csv \
  -- python3 bench.py --gpus 1 --steps 20 --warmup 5 --full --secondary-out $OUT/${T}_prof_secondary.json \
  > $OUT/${T}_prof_bench.json 2> $OUT/${T}_prof.err || { tail -30 $OUT/${T}_prof.err; exit 1; }
python3 tools/kernel_trace_summary.py $OUT/${T}_prof $OUT/${T}_prof_by_grid.json > $OUT/${T}_prof_summary.txt \
  || exit 1
find $OUT/${T}_prof -name "*kernel_stats.csv" -exec head -6 {} \;
# the trace itself is large: keep the summaries only
find $OUT/${T}_prof -name "*kernel_trace.csv" -delete
