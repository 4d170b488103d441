#!/bin/bash
# A/B of the training step and the forward with the encoder convolutions on the exact-fp32 chain vs the bf16x3 route
# usage: bash tools/x3_step_ab.sh [output directory]
O=${1:-${TMPDIR:-/tmp}/x3_step_ab}; mkdir -p $O
for p in fp32 bf16x3; do
  python bench.py --full --no-cpu-baseline --no-stem-ab --conv-precision $p > $O/train_$p.json 2> $O/train_$p.err
  python bench.py --full --workload fwd --no-cpu-baseline --conv-precision $p > $O/fwd_$p.json 2> $O/fwd_$p.err
done
python - "$O" <<'PY'
import json, sys
O = sys.argv[1]
for w in ('train','fwd'):
    for p in ('fp32','bf16x3'):
        try:
            d=json.loads(open('%s/%s_%s.json'%(O,w,p)).read().strip().splitlines()[-1])
            print(w,p,d['value'],d['ms_per_step'],d.get('final_loss'),d['roofline'])
        except Exception as e:
            print(w,p,'FAILED',e); print(open('%s/%s_%s.err'%(O,w,p)).read()[-1500:])
PY
