# GPU tests, smoke, default bench (with CPU baseline), per-config bench, rocprof trace + PMC passes.
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
TAG=${1:-r01h}
export OUT=${OUT:-out}  # logs and profiles go here (the scripts called below use it too)
mkdir -p $OUT
echo "== gpu tests" && timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1; rc=$?; tail -1 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || { tail -40 $OUT/pytest_gpu.log; exit $rc; }
echo "== smoke" && timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?; tail -1 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
echo "== bench" && timeout -k 10 300 python bench.py --full > $OUT/bench.log 2>&1; rc=$?; tail -1 $OUT/bench.log; [ $rc -eq 0 ] || exit $rc
echo "== configs" && timeout -k 10 600 python tools/bench_configs.py > $OUT/bench_configs.log 2>&1; rc=$?; grep -v amdgpu $OUT/bench_configs.log | cut -c1-200; [ $rc -eq 0 ] || exit $rc
echo "== prof" && BENCH_ARGS="--steps 5 --warmup 2" timeout -k 10 900 bash tools/gpu_prof.sh $TAG > $OUT/prof.log 2>&1; rc=$?; tail -2 $OUT/prof.log; exit $rc
