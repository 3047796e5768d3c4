#!/bin/bash
# Same-box A/B of the folded LayerNorm (VCX_LN_FOLD=0 | 1): bench.py twice each, interleaved, kernel families only.
#   gpurun -- 'bash tools/lnfold_ab.sh r03p'
tag=${1:-rXX}
mkdir -p gpurun_out
for rep in 1 2; do
  for f in 0 1; do
    VCX_LN_FOLD=$f python bench.py --steps 8 --warmup 2 --full --no-cpu-baseline --no-gpu-legs --no-video --no-extra --no-decode 2>/dev/null | grep '^{' | python -c "
import json,sys
d=json.loads(sys.stdin.read()); k=d['kernel_families']
print('VCX_LN_FOLD=$f rep $rep: %.2f ms/step | gemm %.2f (%d launches) ln %.2f (%d) flash %.2f gn %.2f' % (d['ms_per_step'], k['gemm']['ms_per_step'], k['gemm']['launches_per_step'], k['layernorm']['ms_per_step'], k['layernorm']['launches_per_step'], k['flash_attn']['ms_per_step'], k['groupnorm']['ms_per_step']))"
  done
done | tee gpurun_out/${tag}_lnfold_ab.txt
