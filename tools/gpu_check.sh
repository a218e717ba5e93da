# quick GPU check of the touched kernels: their tests, the global_feat micro-benchmark, one bench line
set -e
OUT=${OUT:-$PWD/bench_out}   # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread ${CHECK_TESTS:-tests/test_gpu_glds.py tests/test_gpu_parity.py} > $OUT/t2.log 2>&1
timeout -k 10 300 python -u tools/bench_glds.py > $OUT/micro2.txt 2>&1
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench2.json 2> $OUT/bench2.err
