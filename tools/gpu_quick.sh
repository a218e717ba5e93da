OUT=${OUT:-$PWD/bench_out}   # where the logs and result lines go
mkdir -p $OUT
timeout -k 10 300 python -u -m pytest tests/test_gpu_wgrad_c5.py -q --timeout 120 --timeout-method thread > $OUT/wc5.log 2>&1; tail -3 $OUT/wc5.log
timeout -k 10 300 python -u -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py -q --timeout 150 --timeout-method thread > $OUT/par.log 2>&1; tail -2 $OUT/par.log
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline > $OUT/b.json 2> $OUT/b.err; tail -1 $OUT/b.json | cut -c 250-330; grep -A14 per-kernel $OUT/b.err
