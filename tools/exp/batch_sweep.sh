#!/bin/bash
OUT=${OUT:-bench_runs}; mkdir -p $OUT  # where the runs below write
# development aid: the primary bench line for several batch sizes (streams per GPU)
for n in "$@"; do
  python bench.py --full --streams $n --steps 100 --warmup 5 --no-fixed-batch --no-cpu-baseline --no-other-workloads > $OUT/bs_$n.json 2> $OUT/bs_$n.err || tail -2 $OUT/bs_$n.err
  python - <<P
import json
d=json.load(open('$OUT/bs_$n.json')); r=d['roofline']
f=lambda m:[round(v,3) for v in m.values()]
print('$n', '%.2f M frames/s'%(d['value']/1e6), 'ms/step %.3f'%d['ms_per_step'], 'serial', f(r['serial_stage_ms']))
P
done
