#!/bin/bash
# dev: the frame / window kernels with and without the XCD-aware tile order (SRX_XCD_FRAME), one box
for lib in default "$@" default; do
    if [ "$lib" = default ]; then unset SRX_LIB; else export SRX_LIB=$lib; fi
    for wl in "c3_mono 1 f32" "c3_mono 8 f32" "c3_mono_measured 1 f32" "c3_mono 1 f64" "c3_f4 1 f32" "c3_f4 8 f32"; do
        set -- $wl
        python3 bench.py --full --workload $1 --batch $2 --precision $3 --no-cpu-baseline --no-secondary --steps 5 --warmup 2 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('${lib##*/}', '$1 x$2 $3', d['config']['path'], 'ms/step', d['ms_per_step'], 'iter us', d['roofline']['iteration_kernels_us'], 'frac', d['roofline']['frac'])"
    done
done
