#!/bin/bash
# summary of a tools/gpu_check.sh run (local side; the same $OUT, default bench_out/)
T=$1
OUT=${OUT:-bench_out}
tail -1 $OUT/probe_$T.log 2>/dev/null; tail -n 1 $OUT/gpu_tests_$T.log 2>/dev/null
for f in $OUT/b_${T}_4g.json $OUT/b_${T}_zipf.json; do
  [ -f $f ] && python3 -c "import json;d=json.load(open('$f'));print('$f',d['value'],d['kernel_ms'],d['roundtrip_bit_exact'])"
done
