#!/usr/bin/env python3
"""saa_bits.py -- the bits of shift_and_add on the mosaic path (k_saa_tile, k_saa_shift) as hashes: the check of a change to those kernels
that must not change a result.  Every case of tests/test_gpu_saa_group_stage.py (its frame sets on its shapes, the same seeded frames) and
C2 (1024 patches of 64 x 64 at x4, the 16 phases), each in float32 and float64, prints the SHA-256 of its output.  Run it once per build and
compare the listings:

    SRX_LIB=old/libsrx.so python tools/saa_bits.py > old.txt;  python tools/saa_bits.py > new.txt;  diff old.txt new.txt
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sr_mi355x as S  # noqa: E402
from sr_mi355x import synth  # noqa: E402
import test_gpu_saa_group_stage as cases  # noqa: E402

C2_B = 1024


def digest(lr, shifts, prec):
    out = S.shift_and_add_batched(torch.tensor(lr), shifts, 4, precision=prec)
    torch.cuda.synchronize()
    assert S.last_path() == "mosaic", S.last_path()
    return hashlib.sha256(np.ascontiguousarray(out.cpu().numpy()).tobytes()).hexdigest()


def main():
    for shape, frames in cases.CASES:
        shifts, lr, _ = cases._case(shape, frames)
        for prec in ("f32", "f64"):
            print(f"{shape} {frames} {prec}: {digest(lr, shifts, prec)}", flush=True)
    lr = np.rint(np.random.default_rng(4000).uniform(0, 255, (C2_B, 16, 64, 64)))
    for prec in ("f32", "f64"):
        print(f"c2 B={C2_B} {prec}: {digest(lr, synth.phase_shifts(4), prec)}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
