#!/usr/bin/env python3
"""block_bits.py -- the bits of every kernel family built on csrc/srx_block.hpp, as hashes: the check of a change to the block
primitives that must not change a result.  A fixed, seeded list of small ibp calls (3 iterations each: first / steady / last, both
ping-pong planes), each on the path it is meant for (asserted), prints the SHA-256 of the final state and of the MSE trace.  Run it
once per build and compare the listings:

    SRX_LIB=old/libsrx.so python tools/block_bits.py > old.txt;  python tools/block_bits.py > new.txt;  diff old.txt new.txt
    python tools/block_bits.py --plan      # no GPU: the path the library would route every case to
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from sr_mi355x import _lib, synth  # noqa: E402

GRID16 = synth.phase_shifts(4)
GRID12 = [s for i, s in enumerate(GRID16) if i not in (1, 6, 11, 12)]  # one phase less in every row and column: a count PLANE
PSFS = {"gauss": synth.gaussian_psf, "core5": synth.asymmetric_psf, "full7": synth.full_support_psf}

# (name, path, precision, B, f, LR h, LR w, shifts, PSF, samples)
CASES = [(f"patch {fn} {sn} {pn}", "patch", "f32", 3, 4, 64, 64, sh, pn, sn)
         for fn, sh in (("grid16", GRID16), ("grid12", GRID12)) for sn in ("u8", "frac") for pn in ("gauss", "core5", "full7")]
CASES += [(f"stile {fn}", "stile", "f64", 3, 4, 64, 64, sh, "gauss", "u8") for fn, sh in (("grid16", GRID16), ("grid12", GRID12))]
CASES += [(f"dtile {pn}", "dtile", "f32", 1, 4, 64, 48, GRID16, pn, "u8") for pn in ("gauss", "core5")]
CASES += [("ztile", "ztile", "f32", 1, 2, 72, 140, synth.NOMINAL_5, "gauss", "u8"), ("ctile", "ctile", "f64", 1, 2, 72, 140, synth.NOMINAL_5, "gauss", "u8"),
          ("btile", "btile", "f32", 1, 2, 32, 32, synth.MEASURED_4, "gauss", "u8"), ("atile", "atile", "f32", 1, 4, 40, 50, GRID16, "gauss", "u8")]


def planned(prec, sh, psf, h, w, f):
    sh = np.ascontiguousarray(np.asarray(sh, dtype=np.float64))
    k = np.ascontiguousarray(psf)
    return _lib.load().srx_ibp_path_for(8 if prec == "f64" else 4, len(sh), h, w, h * f, w * f, f, sh.ctypes.data_as(_lib._HD),
                                        k.ctypes.data_as(_lib._HD), k.shape[0], k.shape[1], 0).decode()


def main(argv):
    plan_only = "--plan" in argv
    if not plan_only:
        import torch
        from sr_mi355x import api as S
    bad = 0
    for i, (name, want, prec, B, f, h, w, sh, pn, sn) in enumerate(CASES):
        psf = PSFS[pn]()
        if plan_only:
            got = planned(prec, sh, psf, h, w, f)
            print(f"{name}: {got}" + ("" if got == want else f"  (WANTED {want})"))
            bad += got != want
            continue
        rng = np.random.default_rng(1000 + i)
        lr = np.rint(rng.uniform(0, 255, (B, len(sh), h, w)))
        if sn == "frac":
            lr = lr * 0.75 + 0.3
        hr0 = rng.uniform(0, 255, (B, h * f, w * f))
        hr, err = S.ibp_batched(lr, sh, psf, hr0, f, 3, 0.5, precision=prec)
        torch.cuda.synchronize()
        assert S.last_path() == want, (name, S.last_path())
        digest = [hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for t in (hr, err)]
        print(f"{name}: path={want} state={digest[0]} trace={digest[1]}", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
