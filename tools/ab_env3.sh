#!/bin/bash
# same-box comparison of environment settings, step time only (no roofline replays): tools/ab_env3.sh "A=1 B=2" "A=0" ... (three rounds)
OUT=${OUT:-${TMPDIR:-/tmp}}       # bench lines and logs of the runs
for i in 1 2 3; do
for S in "$@"; do
env $S timeout 300 python bench.py --full --no-cpu-baseline --no-roofline --steps 40 --warmup 10 > $OUT/abe.json 2> $OUT/abe.err
python -c "
import json; d=json.loads(open('$OUT/abe.json').read().strip().splitlines()[-1]); print('$S |', d['value'], d['ms_per_step'], d.get('secondary', {}).get('ms_per_step'))"
done
done
