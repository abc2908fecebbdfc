set -u
cd "$(dirname "$0")/.."
R="$PWD"
O="$R/${HLGS_OUT:-out}"
mkdir -p "$O/prof"
timeout -k 10 900 python -m pytest tests -q -m gpu -p no:cacheprovider > "$O/pytest2.log" 2>&1
rc=$?
echo "pytest rc=$rc"; tail -25 "$O/pytest2.log"
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python __graft_entry__.py smoke > "$O/smoke2.log" 2>&1; echo "smoke rc=$?"; tail -3 "$O/smoke2.log"
timeout -k 10 400 python bench.py --full > "$O/bench2.log" 2>&1; rc=$?; echo "bench rc=$rc"; tail -2 "$O/bench2.log"
if [ $rc -ne 0 ]; then exit $rc; fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof" -o r1 -- python3 "$R/bench.py" --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > "$O/prof_bench.log" 2>&1
echo "rocprof rc=$?"
find "$O/prof" -name "*stats*" | head
