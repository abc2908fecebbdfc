set -u
cd "$(dirname "$0")/.."
O=${HLGS_OUT:-out}
mkdir -p $O
timeout -k 10 900 python -m pytest tests/test_gpu_parity.py -q -m gpu -p no:cacheprovider > $O/pytest1.log 2>&1
rc=$?
echo "pytest rc=$rc"
tail -30 $O/pytest1.log
if [ $rc -eq 0 ] || [ $rc -eq 1 ]; then
  timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > $O/bench1.log 2>&1
  echo "bench rc=$?"
  tail -5 $O/bench1.log
fi
