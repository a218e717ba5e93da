#!/bin/bash
# Round-4 evidence at one build (repo root, GPU box): the GPU suite, smoke(), the default bench
# line with its per-kernel table, then tools/profile_round.sh (trace + PMC passes) for it.
# Usage: tools/evidence_r04.sh <tag> [bench.py args]
set -e
TAG=${1:-r04}
shift || true
OUT=${OUT:-$PWD/bench_out}   # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -v -rP --timeout 150 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1
tail -1 $OUT/pytest_gpu_$TAG.log
timeout -k 10 150 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke_$TAG.log 2>&1
tail -1 $OUT/smoke_$TAG.log
timeout -k 10 400 python -u bench.py --full "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_${TAG}_kernels.txt
cat $OUT/bench_$TAG.json
bash tools/profile_round.sh $TAG "$@" > $OUT/profile_$TAG.log 2>&1
head -14 profiles/rocprof_$TAG.md
