#!/bin/bash
# Full GPU suite, smoke() and the default bench line at HEAD (run from the repo root on the box)
set -e
TAG=${1:-r02c}
OUT=${OUT:-$PWD/bench_out}   # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 700 python -u -m pytest tests -m gpu -v -rP --timeout 150 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1
tail -2 $OUT/pytest_gpu_$TAG.log
timeout -k 10 150 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 400 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
cat $OUT/bench_$TAG.json
