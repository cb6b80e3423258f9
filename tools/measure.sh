set -e
# run from the repository root; results go to $OUT (default build/measure, which git ignores)
OUT=${OUT:-build/measure}
mkdir -p "$OUT" && export TMPDIR=/tmp
rm -rf "$OUT"/prof "$OUT"/pmcF "$OUT"/pmcW  # (also clear them locally before merging)
timeout -k 10 600 python bench.py --full > "$OUT"/bench_repeat.json 2> "$OUT"/bench_repeat.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT"/prof --output-format csv -- python3 bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > "$OUT"/bench_prof.json 2> "$OUT"/bench_prof.err
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE -d "$OUT"/pmcF --output-format csv -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > "$OUT"/pmcF.json 2> "$OUT"/pmcF.err
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE -d "$OUT"/pmcW --output-format csv -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > "$OUT"/pmcW.json 2> "$OUT"/pmcW.err
timeout -k 10 600 python bench.py --full --corpus text > "$OUT"/bench_text.json 2> "$OUT"/bench_text.err
