# full default bench (build + c3 + checks + CPU baselines) -> $OUT/bench_full.log (OUT: default bench_out/)
set -o pipefail
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 900 python -u bench.py --full "$@" > $OUT/bench_full.log 2>&1; rc=$?
tail -2 $OUT/bench_full.log | cut -c1-6000; exit $rc
