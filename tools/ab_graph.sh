#!/bin/bash
# A/B of two builds of the library inside ONE job on the GPU box (boxes differ by up to 10 %): alternating graph-replayed bench runs,
# each under its own environment.  The library reads no switch: build the two commits to compare and name their libraries.
#   bash tools/ab_graph.sh "SPV_LIB_PATH=/path/a/libspv_hip.so" "SPV_LIB_PATH=/path/b/libspv_hip.so" [rounds] [extra bench args]
A="$1"; B="$2"; R="${3:-3}"; shift 3 2>/dev/null
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
for i in $(seq 1 $R); do
  for E in "$A" "$B"; do
    v=$(set -o pipefail; env $E timeout -k 10 600 python3 "$ROOT/bench.py" --full --no-cpu-baseline --variants none --no-roofline --no-every-row --no-dp-sequence --no-script-leg --steps 40 --warmup 10 "$@" 2>/dev/null | python3 -c "import sys,json; r=json.loads(sys.stdin.read()); print(r['ms_per_step'], r['eager']['ms_per_step'])") || { echo "$E : bench failed, stopping"; exit 1; }
    echo "$E : graph/eager ms $v"
  done
done
