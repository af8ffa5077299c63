cd "$(dirname "$0")/../.."; OUT=${1:?usage: bash tools/probes/job_r6_bench.sh <output dir>}; mkdir -p "$OUT"
timeout 900 python bench.py --full 2>$OUT/bench.err | tee $OUT/bench_line.json | cut -c1-400
