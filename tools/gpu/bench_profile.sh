# smoke, the full bench line, a kernel trace, a separate FETCH_SIZE pass, tuning table and phase stamps, written under $OUT (default bench_out/)
cd "$(dirname "$0")/../.."; R=$PWD; export TMPDIR=/tmp; OUT=$(realpath -m "${OUT:-bench_out}"); mkdir -p "$OUT"; rm -rf "$OUT/prof_final" "$OUT/pmc_final"
python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke_final.log" 2>&1
timeout 900 python bench.py --full > "$OUT/bench_final.json" 2> "$OUT/bench_final.err"
cd /tmp
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_final" -- python "$R/bench.py" --steps 5 --warmup 2 > "$OUT/prof_final.log" 2>&1
timeout 600 rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_final" -- python "$R/bench.py" --steps 2 --warmup 1 --no-graph > "$OUT/pmc_final.log" 2>&1
cd "$R"
timeout 300 python tools/tune_quad.py > "$OUT/tune_final.txt" 2>&1
timeout 300 python tools/stamps.py > "$OUT/stamps_final.txt" 2>&1
tail -2 "$OUT/smoke_final.log"; cut -c1-2600 "$OUT/bench_final.json"; cut -c1-160 "$OUT"/prof_final/*/*kernel_stats.csv | head -6; ls "$OUT"/pmc_final/*/
