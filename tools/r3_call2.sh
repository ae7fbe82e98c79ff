#!/bin/bash
OUT=${OUT:-results}   # where the logs and bench lines go
# round 3, call 2: new tests + gradient-parity decomposition + --full bench with other_workloads
set -e
mkdir -p $OUT/r3
python -m pytest tests/test_gpu_dispatch.py tests/test_gpu_bench_ranks.py "tests/test_gpu_distgssr_train.py::test_grads_full_geometry_vs_torch_port_autograd" -x -q -m gpu -s > $OUT/r3/c2_tests.log 2>&1 || { tail -40 $OUT/r3/c2_tests.log; exit 1; }
tail -12 $OUT/r3/c2_tests.log
python bench.py --full > $OUT/r3/c2_bench.json 2> $OUT/r3/c2_bench.err || { tail -20 $OUT/r3/c2_bench.err; exit 1; }
python tools/grad_parity.py $OUT/r3/grad_parity.json > $OUT/r3/grad_parity.log 2>&1 || { tail -20 $OUT/r3/grad_parity.log; exit 1; }
grep -v "^CPU" $OUT/r3/grad_parity.log | tail -30
python - <<PY
import json
j=json.load(open("$OUT/r3/c2_bench.json"))
print(j["value"], j["ms_per_step"], j["roofline"]["frac"])
for o in j["other_workloads"]:
    d=o["dominant_kernel"]
    print(o["config"][:40], round(o["value"],1), round(o["ms_per_step"],2), d["operator"], d["tags"], round(d["avg_launch_us"],1), d.get("frac"), (o.get("all_fp32_mfma") or {}).get("value"))
PY
