set -o pipefail
# Whole GPU check from the repo root: bash tools/gpu/run_all.sh TAG.  GPU suite, the full benchmark
# line (every leg), rocprofv3 kernel stats of the full benchmark.  Results under $OUT (default out/).
TAG=${1:-r1c}
OUT=${OUT:-out}
mkdir -p $OUT/prof_$TAG
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -q -p no:cacheprovider -x --timeout 120 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1; rc=$?
tail -30 $OUT/pytest_gpu_$TAG.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full --steps 10 --warmup 3 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err && cat $OUT/bench_$TAG.json &&
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG/bench.json 2> $OUT/prof_$TAG/bench.err && python3 -c "
import csv,sys
for r in list(csv.DictReader(open('$OUT/prof_$TAG/run_kernel_stats.csv')))[:8]: print(r['Name'][:60], r['Calls'], r['AverageNs'], r['Percentage'])"
