# last tree of round 5: soak of the DMD stage (table builds flat, memory flat, losses finite), then the --full bench line
cd "$(dirname "$0")/../.."; OUT=${1:?usage: bash tools/probes/job_r5_final.sh <output dir>}; mkdir -p "$OUT"
STEPS=120 timeout 600 python tools/probes/soak_dmd.py > $OUT/soak.log 2>&1; echo "soak rc=$?"; tail -8 $OUT/soak.log
timeout 900 python bench.py --full > $OUT/bench.log 2>&1; echo "bench rc=$?"; tail -c 3000 $OUT/bench.log
