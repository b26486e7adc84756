#!/bin/bash
# ON THE GPU BOX: one bench run (--full: it reads the kernel table and roofline), JSON kept under $OUT/quick/<tag>.json
# (OUT defaults to bench_out/ in the repository), one summary line on stdout.
#   usage: scripts/quick_bench.sh <tag> [bench.py arguments ...]
TAG=$1; shift
R=${GRAFT_REPO_ROOT:-$PWD}
O=${OUT:-$R/bench_out}/quick
mkdir -p $O
timeout -k 10 300 python3 $R/bench.py --full --no-cpu-baseline "$@" > $O/$TAG.json 2> $O/$TAG.err || { echo "$TAG FAILED"; tail -5 $O/$TAG.err; exit 1; }
python3 - "$O/$TAG.json" "$TAG" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
k = {n: round(v["mean_ms"], 3) for n, v in d["kernels"].items() if "pwattn" in n and "pack" not in n}
print(sys.argv[2], d["value"], "imp/s", d["ms_per_step"], "ms", d["config"]["launch"], d["roofline"]["kernel"], d["roofline"]["frac"], k)
PY
