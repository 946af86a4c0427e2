#!/bin/bash
# GPU round trip used during development: parity tests, then C3 and C2 bench lines
# (--full: with the per-kernel times printed below).  Output under $OUT (default check_out/).
set -o pipefail
OUT=${OUT:-check_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/tcheck.log 2>&1 || { tail -30 $OUT/tcheck.log; exit 1; }
tail -2 $OUT/tcheck.log
timeout -k 10 300 python3 -u bench.py --full --steps 10 --warmup 3 --cpu-sample 0 "$@" > $OUT/bcheck.json 2> $OUT/bcheck.err || { tail -20 $OUT/bcheck.err; exit 1; }
timeout -k 10 200 python3 -u bench.py --full --workload c2 --steps 10 --warmup 3 --cpu-sample 0 "$@" >> $OUT/bcheck.json 2>> $OUT/bcheck.err || { tail -20 $OUT/bcheck.err; exit 1; }
python3 - $OUT/bcheck.json <<'PY'
import json, sys
for l in open(sys.argv[1]):
    if l.startswith("{"):
        d = json.loads(l)
        print(d["config"]["workload"][:3], d["ms_per_step"], "%.3e" % d["value"], d["path_roofline"]["frac"],
              {k: v["avg_ms"] for k, v in d["kernels"].items()})
PY
