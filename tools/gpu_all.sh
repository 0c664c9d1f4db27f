# MI355X: full -m gpu suite then the default bench line with its extra lines and CPU baselines (--full)
set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -v -s -m gpu --timeout 900 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?
grep -E "passed|failed" $OUT/pytest_gpu.log | tail -2
grep -E "^FAILED|north-star|VJP on|whole-batch|dopri5 full|e2e worst" $OUT/pytest_gpu.log | head -30
[ $rc -ne 0 ] && [ "${CONTINUE_ON_FAIL:-0}" != "1" ] && exit $rc
timeout -k 10 600 python -u bench.py --full --steps 10 --warmup 3 > $OUT/bench.json 2> $OUT/bench.err || exit $?
python3 tools/bench_summary.py $OUT/bench.json
