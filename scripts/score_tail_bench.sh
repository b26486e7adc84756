#!/bin/bash
# ON THE GPU BOX: the three parts of scripts/score_tail_bench.py, each under its own time limit, the next one only after the
# previous one ended well.   usage: scripts/score_tail_bench.sh [out.json]   (default profiles/score_tail.json)
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$R/profiles/score_tail.json}
timeout -k 10 240 python3 $R/scripts/score_tail_bench.py --part a --out $OUT &&
timeout -k 10 300 python3 $R/scripts/score_tail_bench.py --part b --out $OUT &&
timeout -k 10 300 python3 $R/scripts/score_tail_bench.py --part c --out $OUT
