#!/bin/bash
# Interleaved A/B of library variants on the metric line + config 5 (ON the GPU box):
#   bash tools/ab_c5.sh <tag> <rounds> <variant>...
# variant: "default" (the in-tree library), a library path, or NAME=VALUE[,NAME=VALUE]@<library or default>
# (environment settings for that run)
# Every run's JSON line lands in the tag's output directory ($O below) as <variant>.<round>.json (config5.ms_per_frame,
# config5.raster_stages_ms, config5.split_ms; "value" is the metric line).
# What the two retired special-case scripts did:
#   every vlibs/c5_*.so against the default, two rounds:  bash tools/ab_c5.sh c5lib 2 default vlibs/c5_*.so
#   one variant library against the default, two rounds:  bash tools/ab_c5.sh c5ab 2 default vlibs/<variant>.so
set -u -o pipefail
TAG=$1; R=$2; shift 2
O=gpurun_out/$TAG; mkdir -p "$O"
ARGS="--full --steps 20 --warmup 5 --train-steps 0 --no-street --no-config4 --no-coarse-debug --no-cpu-baseline --no-config3 --post-leaves 0"
for r in $(seq 1 "$R"); do
  for v in "$@"; do
    envs=""; lib=$v
    case "$v" in *@*) envs=${v%@*}; lib=${v#*@} ;; esac
    n=$(basename "$lib" .so)${envs:+_$(echo "$envs" | tr ',=' '_-')}
    [ "$lib" != default ] && envs="GSR_LIBRARY=$lib${envs:+,$envs}"
    env $(echo "$envs" | tr ',' ' ') timeout -k 10 300 python3 bench.py $ARGS > "$O/$n.$r.json" 2> "$O/$n.$r.err" || exit 1
  done
done
echo "ab_c5 $TAG done"
