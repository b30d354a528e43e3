#!/bin/bash
# One GPU-box session: parity tests, smoke, bench, rocprofv3 kernel stats.
# Every GPU step has its own time limit; steps are chained with && so the
# first failure ends the call.
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-bench_out} && mkdir -p "$OUT"
STEPS="${1:-tests,smoke,bench,prof}"
run() { echo "== $1" ; }
if [[ $STEPS == *tests* ]]; then
  run tests && timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 240 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 \
    || { tail -30 $OUT/pytest_gpu.log; exit 1; }
  tail -3 $OUT/pytest_gpu.log
fi
if [[ $STEPS == *smoke* ]]; then
  run smoke && timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 \
    || { tail -30 $OUT/smoke.log; exit 1; }
  tail -2 $OUT/smoke.log
fi
if [[ $STEPS == *bench* ]]; then
  run bench && timeout -k 10 300 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err \
    || { tail -30 $OUT/bench.err; exit 1; }
  cat $OUT/bench.json
fi
if [[ $STEPS == *big* ]]; then
  run bench_big && timeout -k 10 300 python bench.py --n 524288 --steps 10 --no-cpu-baseline --no-secondary > $OUT/bench_big.json 2> $OUT/bench_big.err \
    || { tail -30 $OUT/bench_big.err; exit 1; }
  cat $OUT/bench_big.json
fi
if [[ $STEPS == *prof* ]]; then
  run prof && timeout -k 10 300 rocprofv3 --kernel-trace --stats -T -d $OUT/prof -o run --output-format csv \
      -- python3 bench.py --no-cpu-baseline --no-secondary --steps 10 > $OUT/bench_prof.json 2> $OUT/prof.err \
    || { tail -30 $OUT/prof.err; exit 1; }
  find $OUT/prof -name "*stats*" | head
  for f in $(find $OUT/prof -name "*kernel_stats.csv"); do cat "$f"; done
fi
if [[ $STEPS == *sq* ]]; then
  run "pmc SQ" && timeout -k 10 300 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_VMEM SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU -T -d $OUT/pmc_SQ -o run --output-format csv \
      -- python3 bench.py --no-cpu-baseline --no-secondary --steps 3 --warmup 1 > $OUT/pmc_SQ.json 2> $OUT/pmc_SQ.err \
    || { tail -30 $OUT/pmc_SQ.err; exit 1; }
fi
if [[ $STEPS == *fullprof* ]]; then
  # the whole benchmark (python bench.py --full, defaults) under the kernel trace
  run fullprof && timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/fullprof -o run --output-format csv \
      -- python3 bench.py --full > $OUT/bench_fullprof.json 2> $OUT/fullprof.err \
    || { tail -30 $OUT/fullprof.err; exit 1; }
  python3 tools/kernel_trace_summary.py $OUT/fullprof $OUT/fullprof_by_grid.json > $OUT/fullprof_summary.txt
fi
if [[ $STEPS == *verifypmc* ]]; then
  # three counter passes of the C2 verify call -> profiles JSON tied to this build
  run "pmc SQ" && timeout -k 10 -s KILL 240 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VALU -T -d $OUT/vp/pmc_SQ -o run --output-format csv \
      -- python3 bench.py --no-cpu-baseline --no-secondary --steps 3 --warmup 1 > $OUT/vp_sq.json 2> $OUT/vp_sq.err \
    || { tail -30 $OUT/vp_sq.err; exit 1; }
  for c in FETCH_SIZE WRITE_SIZE; do
    run "pmc $c" && timeout -k 10 -s KILL 240 rocprofv3 --pmc $c -T -d $OUT/vp/pmc_$c -o run --output-format csv \
        -- python3 bench.py --no-cpu-baseline --no-secondary --steps 3 --warmup 1 > $OUT/vp_$c.json 2> $OUT/vp_$c.err \
      || { tail -30 $OUT/vp_$c.err; exit 1; }
  done
  python3 tools/pmc_verify.py $OUT/vp 65536 $OUT/verify_pmc.json > /dev/null && echo "verify_pmc ok"
fi
if [[ $STEPS == *pmc* ]] && [[ $STEPS != *verifypmc* ]]; then
  for c in FETCH_SIZE WRITE_SIZE; do
    run "pmc $c" && timeout -k 10 300 rocprofv3 --pmc $c -T -d $OUT/pmc_$c -o run --output-format csv \
        -- python3 bench.py --no-cpu-baseline --no-secondary --steps 3 --warmup 1 > $OUT/pmc_$c.json 2> $OUT/pmc_$c.err \
      || { tail -30 $OUT/pmc_$c.err; exit 1; }
  done
  find $OUT -path "*pmc_*" -name "*.csv" | head
fi
if [[ $STEPS == *latprobe* ]]; then
  run latprobe && timeout -k 10 300 python3 tools/lat_probe.py > $OUT/lat_probe.jsonl 2> $OUT/lat_probe.err \
    || { tail -30 $OUT/lat_probe.err; exit 1; }
  cat $OUT/lat_probe.jsonl
fi
if [[ $STEPS == *onlytests* ]]; then
  run onlytests && timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread $TESTS > $OUT/pytest_sel.log 2>&1 \
    || { tail -40 $OUT/pytest_sel.log; exit 1; }
  tail -15 $OUT/pytest_sel.log
fi
if [[ $STEPS == *vlat* ]]; then
  run vlat && timeout -k 10 120 python3 tools/vlat_trace.py run > $OUT/vlat_trace.jsonl 2> $OUT/vlat_trace.err \
    || { tail -30 $OUT/vlat_trace.err; exit 1; }
  cat $OUT/vlat_trace.jsonl
fi
