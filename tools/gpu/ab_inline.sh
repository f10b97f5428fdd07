# Same-box timing of the C4 step forms: two launches (split off: agents +
# PF), the list form (split on, PGW_STEP_LIST=1: k_coord_step_od + the list
# kernel) and the one-launch form (split on: the inline wave solve).
# usage: bash tools/gpu/ab_inline.sh [STEPS]
set -o pipefail
cd "$GRAFT_REPO_ROOT"
STEPS=${1:-286}
mkdir -p gpurun_out/ab
for r in 1 2 3; do
  for v in "off 0" "on 1" "on 0"; do
    set -- $v
    PGW_STEP_LIST=$2 timeout -k 10 300 python -u bench.py --full --steps $STEPS --warmup 20 --no-cpu-baseline --no-variants \
      --pf-split $1 > gpurun_out/ab/inl_$1_$2_$r.log 2>&1 || exit $?
    grep '"metric"' gpurun_out/ab/inl_$1_$2_$r.log | python3 -c "
import sys, json
d = json.loads(sys.stdin.read())
print('split=$1 list=$2', 'us/step %.2f' % (d['ms_per_step'] * 1e3), 'episode %.2f' % (d['ms_per_step_episode'] * 1e3),
      ' '.join('%s %.2f' % (n, x['avg_us']) for n, x in d['kernels'].items()))"
  done
done
