#!/bin/bash
OUT=${OUT:-results}   # where the logs and bench lines go
# the driver's round-end checks, rehearsed: full GPU suite, smoke, --full bench
set -e
mkdir -p $OUT/r3
python -m pytest tests -x -q -m gpu > $OUT/r3/full_gpu_tests.log 2>&1 || { tail -40 $OUT/r3/full_gpu_tests.log; exit 1; }
tail -3 $OUT/r3/full_gpu_tests.log
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2
python bench.py --full > $OUT/r3/full_bench.json 2> $OUT/r3/full_bench.err; python -c "
import json; j=json.load(open('$OUT/r3/full_bench.json')); print(j['value'], j['ms_per_step'], j['all_fp32_mfma']['value'], [ (round(o['value'],1), round(o['ms_per_step'],2)) for o in j['other_workloads']], j['cpu_baseline']['value'])"
