#!/bin/bash
OUT=${OUT:-results}   # where the logs and bench lines go
# round 3, call 7: k_epi_b3 third form (per-view barriers, DPP shift, t registers as stage-2 operand)
set -e
mkdir -p $OUT/r3
python -m pytest tests/test_gpu_b3_accuracy.py tests/test_gpu_distgssr.py tests/test_gpu_bwd_ops.py -x -q -m gpu > $OUT/r3/c7_tests.log 2>&1 || { tail -40 $OUT/r3/c7_tests.log; exit 1; }
tail -2 $OUT/r3/c7_tests.log
for i in 1 2; do
python bench.py --full --no-cpu-baseline --no-other-workloads > $OUT/r3/c7_bench_$i.json 2>> $OUT/r3/c7_bench.err
python - <<PY
import json
j=json.load(open("$OUT/r3/c7_bench_$i.json"))
print("headline", round(j["value"],1), round(j["ms_per_step"],3), round(j["all_fp32_mfma"]["value"],1), {k: round(v,3) for k,v in j["kernel_ms_per_step"].items()})
PY
done
python -m pytest tests/test_gpu_distgssr_train.py -x -q -m gpu > $OUT/r3/c7_train_tests.log 2>&1 || { tail -40 $OUT/r3/c7_train_tests.log; exit 1; }
tail -2 $OUT/r3/c7_train_tests.log
python bench.py --workload train --steps 10 > $OUT/r3/c7_train.json 2>> $OUT/r3/c7_bench.err; python -c "
import json; j=json.load(open('$OUT/r3/c7_train.json')); print('train', j['value'], j['ms_per_step'])"
