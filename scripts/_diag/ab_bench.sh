#!/bin/bash
# A/B of library builds on ONE box (box-to-box spread is larger than most kernel effects): product, each variant, product again.
#   usage: ab_bench.sh "<bench args>" variant1 [variant2 ...]      (variants: scripts/_diag/libnrm_<name>.so; JSON under $OUT, default bench_out/)
ARGS=$1; shift
O=${OUT:-bench_out}; mkdir -p $O
for v in product "$@" product; do
  if [ $v = product ]; then unset NRM_HOTPATH_LIB; else export NRM_HOTPATH_LIB=scripts/_diag/libnrm_$v.so; fi
  python bench.py --full --no-cpu-baseline $ARGS > $O/ab_$v.json 2> $O/ab_$v.err
  python - <<PY
import json
d=json.loads(open("$O/ab_$v.json").read().strip().splitlines()[-1])
k=d["kernels"]
print("$v", d["ms_per_step"], d["config"]["launch"], {n:round(k[n]["mean_ms"],4) for n in k if k[n]["mean_ms"] > 0.15})
PY
done
