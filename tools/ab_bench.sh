#!/bin/bash
# A/B of two library builds on ONE box (boxes differ by several per cent): the current build against adapted_amd/lib/dbg/prev.so
# (a developer's copy of an earlier build), alternating, same bench arguments.  usage: tools/ab_bench.sh [bench.py arguments]
# With PREV_TREE=DIR the "prev" runs are DIR's own bench.py, Python and library (an export of an earlier commit, built): the form for
# a change whose Python binding asks the library for symbols an earlier build does not have.
# Every run has a time limit of its own (AB_TIMEOUT seconds, default 600), and the first run that fails ends the script: nothing
# is started on a GPU behind a run that faulted or hung.
set -o pipefail
ARGS="${@:---no-secondary --steps 6 --warmup 2 --cpu-sample 0}"
for rep in 1 2; do
  for which in prev cur; do
    if [ $which = prev ]; then export ADAPTED_HIP_LIB=$PWD/adapted_amd/lib/dbg/prev.so; else unset ADAPTED_HIP_LIB; fi
    (if [ $which = prev ] && [ -n "$PREV_TREE" ]; then unset ADAPTED_HIP_LIB; cd "$PREV_TREE"; fi; timeout -k 10 ${AB_TIMEOUT:-600} python bench.py $ARGS 2>/dev/null) | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); k=d['kernel_ms']
print('$which', round(d['value']), 'ms/step %.2f' % d['ms_per_step'], 'rows', str(d.get('rows_sha256'))[:16], ' '.join('%s=%.2f' % (n.replace('k_',''), k[n]) for n in list(k)[:13]))" || exit 1
  done
done
