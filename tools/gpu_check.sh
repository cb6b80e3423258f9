# GPU suite (optionally a -k selection) + the full bench (sub-records, CPU baseline) on the current tree.
# usage: bash tools/gpu_check.sh [pytest -k expression]
# run from the repository root; results go to $OUT (default build/measure, which git ignores)
set -e
OUT=${OUT:-build/measure}
mkdir -p "$OUT" && export TMPDIR=/tmp
SEL=${1:+-k "$1"}
timeout -k 10 900 python -u -m pytest tests/ -m gpu -x -v --timeout 300 --timeout-method thread $SEL > "$OUT"/gpu_tests.log 2>&1 || { tail -40 "$OUT"/gpu_tests.log; exit 1; }
tail -3 "$OUT"/gpu_tests.log
timeout -k 10 600 python bench.py --full > "$OUT"/bench_check.json 2> "$OUT"/bench_check.err || { tail -20 "$OUT"/bench_check.err; exit 1; }
head -c 1500 "$OUT"/bench_check.json; echo
