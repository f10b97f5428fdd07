# Kernel-trace timeline of the bench (--full: headline + variants): idle gaps
# between dispatches.  Output goes to $PGW_OUT_DIR (default: bench_out/).
set -o pipefail
cd "$(dirname "${BASH_SOURCE[0]}")/../.."
ROOT=$PWD
OUT=${PGW_OUT_DIR:-$ROOT/bench_out}; mkdir -p "$OUT/prof"
TAG=${1:-gap}
cd "${TMPDIR:-/tmp}" && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$OUT/prof/$TAG" -o run -- python3 "$ROOT/bench.py" --full --steps 100 --warmup 10 --no-cpu-baseline > "$OUT/prof_$TAG.log" 2>&1 || exit $?
cd "$ROOT"
f=$(find "$OUT/prof/$TAG" -name "*kernel_trace.csv" | head -1)
python tools/gpu/gap_trace.py "$f" | tee "$OUT/gaps_$TAG.txt"
