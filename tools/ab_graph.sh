#!/bin/bash
# A/B of two builds inside ONE job on the GPU box (boxes differ by up to 10 %): alternating graph-replayed bench runs, each under its
# own environment.  The library reads no switch: build the two commits to compare and name them.  Two forms of a side:
#   "SPV_LIB_PATH=/path/libspv_hip.so"   a second build of the SAME ABI, run under this checkout's Python
#   "TREE=/path/to/checkout"             a whole checkout (built in place) -- its own bench.py, package and library: for changes that
#                                        touch the host side or the ABI as well
#   bash tools/ab_graph.sh "TREE=/path/parent" "TREE=$PWD" [rounds] [extra bench args, e.g. --steps 400]
#   bash tools/ab_graph.sh "TREE=<checkout of the parent commit, built>" "TREE=$PWD" 5 --steps 400 --no-base224   # a commit against its parent
#                                        (profiles/prologue_v1_ab_graph.txt, profiles/token_embed_v1_ab_graph.txt); a gain counts when
#                                        every run of the second side lies below every run of the first
A="$1"; B="$2"; R="${3:-3}"; shift 3 2>/dev/null
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
for i in $(seq 1 $R); do
  for E in "$A" "$B"; do
    case "$E" in TREE=*) BENCH="${E#TREE=}/bench.py"; ENV="";; *) BENCH="$ROOT/bench.py"; ENV="$E";; esac   # (env with no assignment just runs the command)
    v=$(set -o pipefail; env $ENV timeout -k 10 600 python3 "$BENCH" --full --no-cpu-baseline --variants none --no-roofline --no-every-row --no-dp-sequence --no-script-leg --steps 40 --warmup 10 "$@" 2>/dev/null | python3 -c "import sys,json; r=json.loads(sys.stdin.read()); print(r['ms_per_step'], r['eager']['ms_per_step'])") || { echo "$E : bench failed, stopping"; exit 1; }
    echo "$E : graph/eager ms $v"
  done
done
