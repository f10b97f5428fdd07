# rocprofv3 kernel-trace summary of a short bench run (+ a quick parity check
# and the whole bench, variants included, first).  Output goes to $PGW_OUT_DIR
# (default: bench_out/).
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/../.."
ROOT=$PWD
OUT=${PGW_OUT_DIR:-$ROOT/bench_out}; mkdir -p "$OUT/prof"
TAG=${1:-run}
timeout -k 10 300 python -m pytest tests -m gpu -x -q > "$OUT/pytest_gpu_$TAG.log" 2>&1; rc=$?
tail -3 "$OUT/pytest_gpu_$TAG.log"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --steps 286 --warmup 20 --no-cpu-baseline > "$OUT/bench_$TAG.log" 2>&1 || exit $?
tail -1 "$OUT/bench_$TAG.log"
# (the trace: the headline's steps alone, a plain run)
cd "${TMPDIR:-/tmp}" && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof/$TAG" -o run -- python3 "$ROOT/bench.py" --steps 100 --warmup 10 > "$OUT/prof_$TAG.log" 2>&1 || exit $?
cd "$ROOT"
find "$OUT/prof/$TAG" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$OUT/kernel_stats_$TAG.csv"
cut -c1-200 "$OUT/kernel_stats_$TAG.csv" | head -20
