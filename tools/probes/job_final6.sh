cd "$(dirname "$0")/../.."; OUT=${1:?usage: bash tools/probes/job_final6.sh <output dir>}; mkdir -p "$OUT"
timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -8 | tee $OUT/gpu_suite.txt
timeout 600 python bench.py --full 2>$OUT/bench.err | tee $OUT/bench_line.json
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -5 | tee $OUT/smoke.txt
