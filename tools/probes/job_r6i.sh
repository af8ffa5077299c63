cd "$(dirname "$0")/../.."; OUT=${1:?usage: bash tools/probes/job_r6i.sh <output dir>}; mkdir -p "$OUT"
timeout 900 python -m pytest tests/test_gpu_dist.py -x -q 2>&1 | tail -5 | tee $OUT/tests.txt
timeout 900 python bench.py --full > $OUT/bench.log 2>&1; tail -1 $OUT/bench.log > $OUT/bench_line.json; python - $OUT/bench_line.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read())
for k in ("value","ms_per_step","roofline","roofline_wgrad","linear_gemm","comm_n1","c3_dmd_cycle","c4_diffusion_step","gan_step","kl_mmd"):
    print(k, json.dumps(d.get(k))[:600])
PY
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
