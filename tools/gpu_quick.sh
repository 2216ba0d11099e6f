#!/bin/bash
# quick GPU check: parity tests + bench lines for configs 2-5 (no CPU baseline)
set -o pipefail
export RUN_OUT=${RUN_OUT:-run_out}   # where this script writes
mkdir -p $RUN_OUT
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $RUN_OUT/q_tests.log 2>&1 || { tail -30 $RUN_OUT/q_tests.log; exit 1; }
tail -1 $RUN_OUT/q_tests.log
for c in config2 config3 config4 config5; do
  timeout -k 10 200 python bench.py --full --no-cpu --no-callers --config $c > $RUN_OUT/q_$c.json || exit 1
done
python - <<'PY'
import json, os
for c in ("config2", "config3", "config4", "config5"):
    d = json.load(open(os.path.join(os.environ["RUN_OUT"], f"q_{c}.json")))
    print(c, round(d["value"]), "QP/s", round(d["kernel_ms_avg"], 4), "ms", round(d["roofline"]["frac"], 4), "iters", round(d["iters_mean"], 2), d["iters_max"])
PY
