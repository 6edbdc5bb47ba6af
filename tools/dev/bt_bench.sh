#!/bin/bash
# dev: correctness check + the two c3_rgb bench legs in one run; logs and bench lines go to the directory given: bt_bench.sh OUT_DIR
set -o pipefail
OUT=${1:?usage: bt_bench.sh OUT_DIR}
mkdir -p "$OUT"
timeout -k 10 300 python tools/dev/bt_check.py > "$OUT/bt_check.log" 2>&1 || { tail -5 "$OUT/bt_check.log"; exit 1; }
grep -c "bad=0" "$OUT/bt_check.log"; grep -v "bad=0" "$OUT/bt_check.log" | grep -v tiles | head
timeout -k 10 200 python bench.py --full --workload c3_rgb --no-cpu-baseline --no-secondary > "$OUT/bt_b1.json" 2> "$OUT/bt_b1.err" &&
timeout -k 10 200 python bench.py --full --workload c3_rgb --batch 8 --no-cpu-baseline --no-secondary > "$OUT/bt_b8.json" 2>> "$OUT/bt_b1.err"
python - "$OUT" <<'PY'
import json, os, sys
for f in ("bt_b1.json", "bt_b8.json"):
    j=json.loads(open(os.path.join(sys.argv[1], f)).read().strip().splitlines()[-1]); print(j["config"]["path"], j["ms_per_step"], j["roofline"]["frac"], j["roofline"]["iteration_kernels_us"], j["sane"])
PY
