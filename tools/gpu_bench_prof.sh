# Bench (default + T=64 variant) and rocprof trace / PMC passes of the default bench.
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${1:-r01g}
export OUT=${OUT:-out}  # logs and profiles go here (the scripts called below use it too)
mkdir -p $OUT
echo "== bench" && timeout -k 10 300 python bench.py --full > $OUT/bench.log 2>&1; rc=$?; tail -1 $OUT/bench.log; [ $rc -eq 0 ] || exit $rc
echo "== bench T64" && timeout -k 10 300 python bench.py --imhk-steps 64 > $OUT/bench_t64.log 2>&1; rc=$?; tail -1 $OUT/bench_t64.log; [ $rc -eq 0 ] || exit $rc
echo "== prof" && BENCH_ARGS="--steps 5 --warmup 2" timeout -k 10 900 bash tools/gpu_prof.sh $TAG > $OUT/prof.log 2>&1; rc=$?; tail -3 $OUT/prof.log; exit $rc
