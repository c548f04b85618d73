#!/bin/bash
# timing-only ablations of k_cand_stats2 (ADP_ABLATE bits 2^20 no finish, 2^21 no sweep B, 2^23 no sweep A); results are wrong when set.
# Only a -DADP_ABLATE build of the library has the mask (common.h: ABLATED); it is made here, from adapted_amd/build.py's flags and both
# translation units, as adapted_amd/lib/dbg/libadapted_hip_ablate.so, and loaded through ADAPTED_HIP_LIB.
# usage: tools/experiments/cs2_ablate.sh [bench.py arguments]   (default: 24 000 reads at the 200 k window)
cd "$(dirname "$0")/../.." || exit 1
ARGS="${@:---primary cnn --reads 24000 --max_obs_trace 200000 --no-secondary --steps 4 --warmup 2 --cpu-sample 0}"
LIB=$PWD/adapted_amd/lib/dbg/libadapted_hip_ablate.so
mkdir -p adapted_amd/lib/dbg
hipcc $(python -c "from adapted_amd import build; print(' '.join(build.FLAGS))") -DADP_ABLATE -Iinclude -Iadapted_amd/csrc -o "$LIB" \
  adapted_amd/csrc/adapted_hip.hip adapted_amd/csrc/modules.hip || exit 1
export ADAPTED_HIP_LIB=$LIB
for a in 0 1048576 2097152 3145728 8388608 11534336; do
ADP_ABLATE=$a python bench.py $ARGS 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d['kernel_ms']
print('abl=$a', 'ms/step %.2f' % d['ms_per_step'], 'cand_stats=%.2f' % k.get('k_cand_stats',0))"
done
