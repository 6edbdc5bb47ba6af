#!/bin/bash
# ab_bench.sh WORKLOAD LIB... -- the same bench leg with several builds of libsrx.so on ONE box (box to box the same build varies by ~6 %):
#   gpurun -- 'bash tools/ab_bench.sh c2 default enph459-super-resolution_amd/build/libsrx_x.so'
# AB_ROUNDS=n (default 1) walks the list n times, so that the builds' runs interleave (2 n runs per build); every run has a time limit
# of its own and the first one that fails ends the script with its status.
set -o pipefail
WL=$1; shift
for round in $(seq 1 ${AB_ROUNDS:-1}); do
    for lib in "$@"; do
        if [ "$lib" = default ]; then unset SRX_LIB; else export SRX_LIB=$lib; fi
        for rep in 1 2; do
            timeout -k 10 ${AB_TIMEOUT:-300} python3 bench.py --full --workload $WL --no-cpu-baseline --no-secondary --steps 5 --warmup 2 2>/dev/null | python3 -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$lib', d['config']['path'], 'ms/step', d['ms_per_step'], 'iter us', d['roofline']['iteration_kernels_us'], 'frac', d['roofline']['frac'])" || exit $?
        done
    done
done
