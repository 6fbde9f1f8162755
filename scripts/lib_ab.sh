#!/bin/bash
# A/B of library builds inside ONE gpurun call (box-to-box variance is several %):  bash scripts/lib_ab.sh <tag> base h2 h16 base ...
# (names: base = the in-tree libmcpc.so, X = scripts/bin/libmcpc_X.so); prints learning / inference us per step of a short bench run.
TAG=$1; shift
OUT=${MCPC_OUT:-out}/$TAG      # output folder (MCPC_OUT overrides its parent)
mkdir -p $OUT
for v in "$@"; do
  L=$PWD/scripts/bin/libmcpc_$v.so; [ $v = base ] && L=$PWD/montecarlopredictivecoding_amd/libmcpc.so
  MCPC_LIB=$L timeout -k 10 200 python3 bench.py --steps ${AB_STEPS:-4} --warmup 1 --no-cpu-baseline --no-self-check --full > $OUT/$v.json 2> $OUT/$v.err; rc=$?
  # (behind its result line bench.py exits 1 when the library is no build of the tree's sources, which an A/B library never is)
  if [ $rc -ne 0 ] && ! { [ $rc -eq 1 ] && [ -s $OUT/$v.json ] && grep -q "not a clean build of this tree" $OUT/$v.err; }; then echo "$v failed (rc=$rc)"; exit 1; fi
  python3 - <<PY
import json
d=json.load(open("$OUT/$v.json"))
print("%-8s learning %.2f us/step  plain-kernel %.2f  inference %.2f" % ("$v", d["config"]["us_per_langevin_step"], d["roofline"]["us_per_step"], d["config"]["inference_only"]["us_per_langevin_step"]))
PY
done
