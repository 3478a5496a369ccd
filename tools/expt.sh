#!/bin/bash
# developer tool: time alternative builds of the library (build/expt/expt_<n>.so, selected through GPUDRIVE_AMD_LIB)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT:-out}
mkdir -p $OUT
for e in "$@"; do
  GPUDRIVE_DEV=1 GPUDRIVE_AMD_LIB=$ROOT/build/expt/expt_$e.so timeout -k 10 200 python bench.py --full --steps 91 --warmup 10 --roofline-steps 91 --no-cpu-baseline --workloads ${WL:-synthetic} > $OUT/expt_$e.log 2>$OUT/expt_$e.err
  python -c "
import json;r=json.loads(open('$OUT/expt_$e.log').read().strip().splitlines()[-1]);print('expt','$e','ms/step %.3f'%r['ms_per_step'],{k:round(v['avg_us']) for k,v in r['kernels'].items()})"
done
