# the full bench line (bench.py --full: every measurement beside the headline) and its log, written under $OUT (default bench_out/)
cd "$(dirname "$0")/../.."; export TMPDIR=/tmp; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 900 python bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"; cut -c1-200 "$OUT/bench_final.json"
