#!/bin/bash
# Same-box A/B of two builds on bench.py's configurations: the builds alternate
# within every round, so drift of the box hits both alike.
# usage: scripts/ab_builds.sh OTHER_TREE OUT_DIR [ROUNDS] [CONFIGS]
#   OTHER_TREE a built checkout of the other commit (bench.py, talos_amd/ with
#              libtlsgpu.so, profiles/pmc_config*.json); this tree is the second
#   OUT_DIR    gets {other,this}_<config>_<round>.json and summary.txt (per
#              config both builds' values, medians and their ratio)
# Every bench run has its own time limit; the first failure ends the script.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OTHER=$1; O=$2; ROUNDS=${3:-5}; CONFIGS=${4:-"B C D"}
mkdir -p $O
for r in $(seq 1 $ROUNDS); do
  for c in $CONFIGS; do
    for b in other this; do
      tree=$R; [ $b = other ] && tree=$OTHER
      timeout -k 10 240 python $tree/bench.py --gpus 1 --config $c --no-cpu-baseline \
        > $O/${b}_${c}_$r.json 2> $O/${b}_${c}_$r.err || exit $?
    done
  done
done
python - $O $CONFIGS <<'PY' | tee $O/summary.txt
import glob, json, statistics, sys
d = sys.argv[1]
for cfg in sys.argv[2:]:
    v = {b: [json.loads([l for l in open(p) if l.startswith("{")][-1])["value"]
             for p in sorted(glob.glob(f"{d}/{b}_{cfg}_*.json"))] for b in ("other", "this")}
    mo, mt = (statistics.median(v[b]) for b in ("other", "this"))
    where = "inside" if min(v["other"]) <= mt <= max(v["other"]) else "above" if mt > mo else "BELOW"
    print(f"config {cfg}: medians other {mo:.2f} this {mt:.2f} GiB/s, this/other {mt / mo:.4f}, "
          f"{where} the other build's spread")
    for b in ("other", "this"):
        print(f"  {b:5s} " + " ".join(f"{x:.2f}" for x in v[b]))
PY
