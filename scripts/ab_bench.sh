#!/bin/bash
# A/B of one environment knob on one machine: scripts/ab_bench.sh KNOB tag [bench args]   -> $AB_OUT/<tag>_{1,0}.jsonl (AB_OUT: default ab_out)
KNOB=$1; TAG=$2; shift 2
O=${AB_OUT:-ab_out}; mkdir -p $O
for v in 1 0 1 0; do
  env $KNOB=$v python bench.py --full --no-cpu-baseline "$@" > $O/${TAG}_$v.json.tmp 2>> $O/${TAG}.err || exit 1
  cat $O/${TAG}_$v.json.tmp >> $O/${TAG}_$v.jsonl
done
python - <<PY
import json
for v in (1, 0):
    for line in open("$O/${TAG}_%d.jsonl" % v):
        d = json.loads(line)
        s = d.get("secondary", {})
        print("${KNOB}=%d" % v, "f32", d["value"], "| bf16", s.get("bf16", {}).get("value"), "| predict b16", s.get("predict_b16", {}).get("f32", {}).get("value"), s.get("predict_b16", {}).get("bf16", {}).get("value"),
              "| b1", s.get("predict_b1", {}).get("f32", {}).get("value"), s.get("predict_b1", {}).get("bf16", {}).get("value"), "| cfg1", s.get("cfg1", {}).get("value"),
              "| cfg5", s.get("cfg5", {}).get("f32", {}).get("value"), s.get("cfg5", {}).get("bf16", {}).get("value"))
PY
