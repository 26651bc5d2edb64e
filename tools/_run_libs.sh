#!/bin/bash
# same-box A/B of whole-library builds: build_variants/<name>/libvb2.so for name in $VARIANTS, alternated ROUNDS times
# (default 2; the reader discards round 1 as warm-up).  Every leg runs under a time limit of its own, and the first leg
# that fails or runs out of time ends the whole run: nothing more is started on a device that may be in trouble.
set -o pipefail
cd "$(dirname "$0")/.."
for rep in $(seq 1 ${ROUNDS:-2}); do
  for v in $VARIANTS; do
    echo "== $v round $rep"
    export VB2_LIB_PATH=$PWD/build_variants/$v/libvb2.so
    timeout -k 10 240 python bench.py --steps 1500 --warmup 200 --no-extras --no-cpu-baseline --no-optimize 2>/dev/null | python -c "import sys,json; d=json.loads(sys.stdin.readline()); print('  headline %.1f k evals/s  %.2f us' % (d['value']/1e3, d['ms_per_step']*1e3))" || exit 1
    timeout -k 10 180 python tools/opt_time.py 2>&1 | grep "M=" || exit 1
    timeout -k 10 180 python tools/quality_profile_time.py 2>&1 | awk '/codes/ && n++ < 2' || exit 1
    VB2_STEPS_ONLY=1 timeout -k 10 240 python tools/cohort_steps.py 2>&1 | grep samples || exit 1
  done
done
