# quick regression loop: GPU tests, per-configuration launch times, the full bench line, stamps; written under $OUT (default bench_out/)
cd "$(dirname "$0")/../.."; export TMPDIR=/tmp; OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout 900 python -m pytest tests -q -m gpu > "$OUT/pytest_gpu20.log" 2>&1
timeout 300 python tools/tune_quad.py > "$OUT/tune20.txt" 2>&1
timeout 900 python bench.py --full --no-cpu-baseline > "$OUT/bench20.json" 2> "$OUT/bench20.err"
timeout 600 python tools/stamps.py > "$OUT/stamps20.txt" 2>&1
tail -3 "$OUT/pytest_gpu20.log"; tail -4 "$OUT/tune20.txt"; cut -c1-330 "$OUT/bench20.json"; grep -A3 "== down" "$OUT/stamps20.txt"
