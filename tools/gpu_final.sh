# round-end refresh: bench (with sub-records), rocprof kernel stats of the bench command, phases
# (run after tools/profile_all.sh run + collect, so bench's traffic keys are current)
# run from the repository root; results go to $OUT (default build/measure, which git ignores)
set -e
OUT=${OUT:-build/measure}
mkdir -p "$OUT" && export TMPDIR=/tmp
rm -rf "$OUT"/prof
timeout -k 10 600 python bench.py --full > "$OUT"/bench_final.json 2> "$OUT"/bench_final.err || { tail -20 "$OUT"/bench_final.err; exit 1; }
head -c 600 "$OUT"/bench_final.json; echo
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT"/prof --output-format csv -- python3 bench.py --steps 5 --warmup 1 > "$OUT"/bench_prof.json 2> "$OUT"/bench_prof.err
find "$OUT"/prof -name "*kernel_stats.csv" | xargs cat | cut -d, -f1-4 | head -8
rm -f "$OUT"/phases.txt
DMX_KINDS=repeat,text timeout -k 10 200 python tools/phases.py "$OUT"/phases.txt > /dev/null 2>&1
cat "$OUT"/phases.txt
