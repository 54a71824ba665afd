# GPU suite + bench lines; output under $O (default check_out/)
#   CFGS="c2 c2_1024 ..." selects the extra bench configs (short runs)
set -o pipefail
cd "$(dirname "$0")/.."
O=${O:-check_out}
mkdir -p $O
if [ -z "$SKIP_TESTS" ]; then
  timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread ${PYTEST_K:+-k "$PYTEST_K"} > $O/pytest_gpu.log 2>&1 || exit 3
fi
# the whole line (CPU baseline, e2e leg): --full
timeout -k 10 300 python bench.py --full > $O/bench.json 2> $O/bench.err || exit 4
for c in ${CFGS}; do
  timeout -k 10 300 python bench.py --config $c --steps 3 --warmup 1 > $O/bench_$c.json 2> $O/bench_$c.err || exit 5
done
