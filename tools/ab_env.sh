#!/bin/bash
# A/B: bench the in-tree library under environment variants. Each line of $AB_VARIANTS
# is "name ENV=value ..." (name alone = defaults).
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
while read -r name envs; do
  [ -z "$name" ] && continue
  env $envs timeout -k 10 200 python bench.py --full --steps 24 --warmup 2 --no-cpu-baseline --roofline-images 1 ${BENCH_ARGS:-} > $OUT/abenv_$name.log 2>&1 || exit $?
  echo "$name $(python -c "import json;d=json.load(open('$OUT/abenv_$name.log'));print(d['ms_per_spp'], d['roofline']['avg_launch_us'], d['roofline']['frac'])")"
done <<< "${AB_VARIANTS}"
