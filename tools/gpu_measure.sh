# Round measurement on one GPU, in two calls (each well under 20 minutes); OUT: output directory
# (default bench_out/ in the repository):
#   PART=a  parity tests (-m gpu), smoke(), the full bench line -> $OUT/{pytest_gpu,smoke,bench}.log
#   PART=b  rocprofv3 kernel-trace stats of a c2 bench run (checks + serializer included), then separate
#           PMC passes (FETCH_SIZE, WRITE_SIZE; one counter group per run) over the build, serializer and
#           query kernels -> $OUT/{prof,pmc_f,pmc_w}; then
#           SME_PMC_BATCHES=40 python tools/pmc_summary.py 1000000 1048576 $OUT/pmc_f $OUT/pmc_w
#           writes profiles/pmc_traffic.json (the first 40 query batches are the headline c3 ones)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; OUT=${OUT:-$R/bench_out}; mkdir -p $OUT
if [ "${PART:-a}" = a ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { echo PYTEST_FAIL; tail -30 $OUT/pytest_gpu.log; exit 1; }
  grep -E "passed|failed" $OUT/pytest_gpu.log | tail -1
  timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { echo SMOKE_FAIL; tail -30 $OUT/smoke.log; exit 1; }
  tail -1 $OUT/smoke.log
  timeout -k 10 900 python -u bench.py --full > $OUT/bench.log 2>&1 || { echo BENCH_FAIL; tail -30 $OUT/bench.log; exit 1; }
  tail -1 $OUT/bench.log | cut -c1-400
  echo MEASURE_A_OK
  exit 0
fi
KRE=${KRE:-"k_tok_fast|k_agg_w|k_rs_scatter|k_rs_count|k_vocab|k_tfsort|k_tf_tile|k_ser_write|k_ser_big|k_query_win|k_query_seed"}
BARGS="--full --steps 1 --warmup 1 --cpu-docs 0 --no-e2e"
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/prof $OUT/pmc_f $OUT/pmc_w
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run -- python3 $R/bench.py --full --steps 3 --warmup 1 --cpu-docs 0 --no-e2e > $OUT/bench_prof.log 2>&1 || { echo PROF_FAIL; tail -20 $OUT/bench_prof.log; exit 1; }
timeout -s KILL 400 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex "$KRE" --output-format csv -d $OUT/pmc_f -o run -- python3 $R/bench.py $BARGS > $OUT/pmc_f.log 2>&1 || { echo PMC_F_FAIL; tail -5 $OUT/pmc_f.log; exit 1; }
timeout -s KILL 400 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex "$KRE" --output-format csv -d $OUT/pmc_w -o run -- python3 $R/bench.py $BARGS > $OUT/pmc_w.log 2>&1 || { echo PMC_W_FAIL; tail -5 $OUT/pmc_w.log; exit 1; }
echo MEASURE_B_OK
