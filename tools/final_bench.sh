#!/bin/bash
# Round-end measurements (GPU box): the driver's --steps 20 line, the default line, and every
# BASELINE config at 16 spp (one JSON line each), each under its own time limit.
set -e
TAG=${TAG:-r06}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full --steps 20 > $OUT/${TAG}_bench_s20.json
timeout -k 10 400 python bench.py --full > $OUT/${TAG}_bench_default.json
: > $OUT/${TAG}_configs.jsonl
for c in cornell coffee "coffee --no-multiscattering" spaceship spaceship_close lamp; do
  timeout -k 10 300 python bench.py --full --config $c --steps 16 --no-cpu-baseline --spaceship-spp 0 >> $OUT/${TAG}_configs.jsonl
done
