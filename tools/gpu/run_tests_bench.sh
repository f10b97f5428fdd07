# build + smoke, the GPU suite, then the whole bench (--full, with a short CPU
# baseline).  Logs go to $PGW_OUT_DIR (default: bench_out/).
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/../.."
OUT=${PGW_OUT_DIR:-bench_out}; mkdir -p "$OUT"
rocm-smi --showproductname > "$OUT/smi.log" 2>&1 || true
timeout -k 10 400 python -c "import __graft_entry__ as g; g.build(); g.smoke()" > "$OUT/smoke.log" 2>&1 || { echo "SMOKE FAILED rc=$?"; tail -40 "$OUT/smoke.log"; exit 1; }
tail -3 "$OUT/smoke.log"
timeout -k 10 600 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu.log" 2>&1; rc=$?
tail -30 "$OUT/pytest_gpu.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --steps 286 --warmup 20 --cpu-sample-envs 1024 --cpu-sample-steps 10 > "$OUT/bench.log" 2>&1; rc=$?
tail -5 "$OUT/bench.log"
exit $rc
