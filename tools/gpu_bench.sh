# full bench + rocprof kernel stats of the plain bench command (developer aid)
# run from the repository root; results go to $OUT (default build/measure, which git ignores)
set -e
OUT=${OUT:-build/measure}
mkdir -p "$OUT" && export TMPDIR=/tmp
rm -rf "$OUT"/bprof
timeout -k 10 600 python bench.py --full > "$OUT"/bench.json 2> "$OUT"/bench.err || { tail -20 "$OUT"/bench.err; exit 1; }
cat "$OUT"/bench.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT"/bprof --output-format csv -- python3 bench.py --steps 5 --warmup 2 > "$OUT"/bench_prof.json 2> "$OUT"/bench_prof.err
find "$OUT"/bprof -name "*kernel_stats.csv" | head -1 | xargs head -8
