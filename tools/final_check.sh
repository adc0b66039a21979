#!/bin/bash
# Round-end check on the GPU box, in the driver's order: the GPU suite, smoke(), then the plain
# bench line (N=1) and the full one (--full).  Each step has its own time limit; the first
# failure ends it.  Usage: bash tools/final_check.sh [output folder, default check_out]
OUT=${1:-check_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
    > $OUT/pytest_final.log 2>&1 || { tail -30 $OUT/pytest_final.log; exit 1; }
tail -1 $OUT/pytest_final.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" \
    > $OUT/smoke_final.log 2>&1 || { tail -30 $OUT/smoke_final.log; exit 1; }
tail -1 $OUT/smoke_final.log
timeout -k 10 200 python -u bench.py --gpus 1 --steps 20 --warmup 5 > $OUT/bench_plain.json 2> $OUT/bench_plain.err \
    || { tail -30 $OUT/bench_plain.err; exit 1; }
cat $OUT/bench_plain.json
timeout -k 10 400 python -u bench.py --full > $OUT/bench_final.json 2> $OUT/bench_final.err \
    || { tail -30 $OUT/bench_final.err; exit 1; }
cat $OUT/bench_final.json
