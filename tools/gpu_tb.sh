# GPU tests, smoke and the default bench (no rocprof).
set -o pipefail
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
export OUT=${OUT:-out}  # logs and profiles go here (the scripts called below use it too)
mkdir -p $OUT
echo "== gpu tests" && timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1; rc=$?; tail -1 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || { tail -40 $OUT/pytest_gpu.log; exit $rc; }
echo "== smoke" && timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; rc=$?; tail -1 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
echo "== bench" && timeout -k 10 300 python bench.py --full ${BENCH_ARGS} > $OUT/bench.log 2>&1; rc=$?; tail -1 $OUT/bench.log | python3 -c "import json,sys; j=json.loads(sys.stdin.read()); print(json.dumps({k: j[k] for k in ('value','ms_per_step','parity_check','certificate_redos','kernel_ms')}))"; exit $rc
