#!/usr/bin/env python3
"""block_bits.py -- the bits of every kernel family built on csrc/srx_block.hpp, as hashes: the check of a change to the block
primitives that must not change a result.  A fixed, seeded list of small ibp calls (3 iterations each: first / steady / last, both
ping-pong planes), each on the path it is meant for (asserted), prints the SHA-256 of the final state and of the MSE trace.  Run it
once per build and compare the listings:

    SRX_LIB=old/libsrx.so python tools/block_bits.py > old.txt;  python tools/block_bits.py > new.txt;  diff old.txt new.txt
    python tools/block_bits.py --plan      # no GPU: the path the library would route every case to

--flags prints a second list instead: one case per place below the entry points that reads a SRX_FLAG_DIAG_* switch of the call, each
run with the flag off and with it on.  A run prints its path (asserted), the SHA-256 of its outputs and the launches per kernel id
(srx_profile_get), so a flag that stops arriving where it is read changes the listing.  Compare the listings of two builds as above
(--flags --plan: the routes, no GPU).

--walk prints a third list: one case per user of the segmented LDS spline walk (fused::walk_pass, csrc/srx_fused.hpp) -- the check of a
change to the walk that must not change a bit.  A case prints its path (asserted; the primitives have none), the SHA-256 of its outputs and
the launches per kernel id, which name the kernels that walked (--walk --plan: the routes, no GPU).
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
# (new cases go to the END: a case's seed is its index)
# the float mosaic of the windows (M8 = false); then two frames per phase -- more than four frames on a near-band pixel, so the group tail of
# patch::near_px runs on every route (the samples' sums pass 255: the float mosaic and a count plane) -- and the windows' count-plane
# instantiation (k_ibp_dtile<false, 3, *>).  --plan prints the path only: it says that GRID12 and GRID16 * 2 stay on "dtile" at this shape.
# That they run the count-plane instantiation follows from their count maps, which are no product of a row and a column mask
# (patch::c01_masks: a phase missing from every row and column; two frames on one phase), so the driver launches <false, ...>
CASES += [(f"dtile {pn} frac", "dtile", "f32", 1, 4, 64, 48, GRID16, pn, "frac") for pn in ("gauss", "core5")]
CASES += [("patch grid16x2", "patch", "f32", 3, 4, 64, 64, GRID16 * 2, "gauss", "u8"), ("patch grid16x2 core5", "patch", "f32", 2, 4, 64, 64, GRID16 * 2, "core5", "u8"),
          ("stile grid16x2", "stile", "f64", 3, 4, 64, 64, GRID16 * 2, "gauss", "u8"), ("dtile grid16x2", "dtile", "f32", 1, 4, 64, 48, GRID16 * 2, "gauss", "u8"),
          ("dtile grid12", "dtile", "f32", 1, 4, 64, 48, GRID12, "gauss", "u8"), ("dtile grid12 frac core5", "dtile", "f32", 1, 4, 64, 48, GRID12, "core5", "frac")]
# HR 272 x 208: two windows on each axis -- three near-band tables -- and no side a multiple of 32: the ragged last tiles of the operand-plane kernel
CASES += [("dtile 2x2 u8", "dtile", "f32", 2, 4, 68, 52, GRID16, "gauss", "u8"), ("dtile 2x2 grid12 frac", "dtile", "f32", 2, 4, 68, 52, GRID12, "core5", "frac")]


# (reader of the flag, call, path, precision, B, f, LR h, LR w, shifts, flags off, flag): the smallest shapes that reach each reader
L = _lib
FLAG_CASES = [("prefilter2d in shift_and_add", "saa", "fused", "f32", 2, 2, 64, 64, synth.NOMINAL_4, L.FLAG_PER_FRAME, L.FLAG_DIAG_NO_PREFILTER_TILE),
              ("prefilter2d below the composed path", "ibp", "composed", "f32", 2, 2, 32, 32, synth.MEASURED_4, L.FLAG_COMPOSED, L.FLAG_DIAG_NO_PREFILTER_TILE),
              ("use_v1", "ibp", "fused", "f64", 2, 2, 32, 32, synth.MEASURED_4, 0, L.FLAG_DIAG_V1),
              ("make_kernel7", "ibp", "btile", "f32", 2, 2, 32, 32, synth.MEASURED_4, 0, L.FLAG_DIAG_NO_SEPARABLE),
              ("mosaic::iterate zero fuse", "ibp", "mosaic", "f32", 2, 2, 72, 140, synth.NOMINAL_5, L.FLAG_TILES, L.FLAG_DIAG_NO_ZERO_FUSE),
              ("patch::builds_itself", "ibp", "patch", "f32", 3, 4, 64, 64, GRID16, 0, L.FLAG_DIAG_NO_ZERO_FUSE),
              ("patch::iterate byte loads", "ibp_u8", "patch", "f32", 3, 4, 64, 64, GRID16, 0, L.FLAG_DIAG_U8_BYTE_LOADS),
              ("mosaic::saa", "saa", "mosaic", "f32", 2, 2, 64, 64, synth.NOMINAL_4, 0, L.FLAG_DIAG_SAA_ONE_PASS),
              ("dtile::plan", "ibp", "dtile", "f32", 1, 4, 64, 80, GRID16, 0, L.FLAG_DIAG_WIDE_WINDOWS)]
FLAGS_HEADER = """# one case per reader of a SRX_FLAG_DIAG_* switch below the entry points; every case with the flag off, then on
# a case ends in 'off != on (what differs)' or in 'off == on'.  On the MI355X one case is indistinguishable by bits and launch counts:
# 'patch::iterate byte loads', whose flag selects another instantiation of k_patch_build (same kernel id, same bits by design); the
# kernel NAMES of a kernel trace of this run tell its two runs apart (k_patch_build<0, unsigned char, true> against <..., false>)
# (SRX_FLAG_DIAG_V1's MSE trace is printed to 10 digits, not hashed: that iteration sums it with atomics, and two runs of one build differ
# in its last bits)"""


# (name, call, path, precision, B, f, LR h, LR w, shifts, PSF, flags).  zoom / shift: one [h, w] image, f = the zoom factor / unused.
HALF2, HALF4 = synth.phase_shifts(2), synth.phase_shifts(4)  # x2 / x4: every HR shift has the fraction one half
WALK_CASES = [("zoom_cubic 70x130 (k_prefilter_tile, mirror ends)", "zoom", None, "f32", 1, 2, 70, 130, None, None, 0),
              ("shift_cubic 70x130 (k_prefilter_tile, reflect ends)", "shift", None, "f32", 1, 1, 70, 130, None, None, 0)]
WALK_CASES += [(f"shift_and_add x{f} {prec} {fn} (k_saa_tile{'' if fl else ', k_saa_shift'})", "saa", "mosaic", prec, 2, f, 64, 64, sh, None, fl)
               for f, sh in ((2, HALF2), (4, HALF4)) for prec in ("f32", "f64") for fn, fl in (("two-pass", 0), ("one-pass", L.FLAG_DIAG_SAA_ONE_PASS))]
WALK_CASES += [("ibp per frame f64 (k_fwd_tile, k_bwd_tile)", "ibp", "fused", "f64", 2, 2, 40, 50, synth.MEASURED_4, "core5", L.FLAG_PER_FRAME),
               ("ibp per frame f32 x3 (k_fwd_tile, k_bwd_tile)", "ibp", "fused", "f32", 2, 3, 40, 50, synth.MEASURED_4, "core5", L.FLAG_PER_FRAME)]
WALK_CASES += [(f"ibp tiles {prec} {pn} (k_fwd_mosaic, k_bwd_mosaic {'separable' if pn == 'gauss' else '7 x 7'})", "ibp", "mosaic", prec, 2, 4, 40, 50, HALF4, pn,
                L.FLAG_TILES) for prec in ("f32", "f64") for pn in ("gauss", "core5")]
WALK_ITERS = 2


def walk_cases(plan_only):
    if not plan_only:
        import torch
        from sr_mi355x import api as S
    lib, bad = _lib.load(), 0
    for i, (name, call, want, prec, B, f, h, w, sh, pn, fl) in enumerate(WALK_CASES):
        if plan_only:
            if want is None:
                print(f"{name}: prefilter2d_fast takes float32 planes of at least 64 x 64 to k_prefilter_tile")
                continue
            got = planned(prec, sh, PSFS[pn or "gauss"](), h, w, f, fl, call)
            print(f"{name} flags={fl:#x}: {got}" + ("" if got == want else f"  (WANTED {want})"))
            bad += got != want
            continue
        rng = np.random.default_rng(3000 + i)
        lib.srx_profile_enable(1)
        if call in ("zoom", "shift"):
            x = np.rint(rng.uniform(0, 255, (1, h, w)))
            outs = (S.zoom_batched(x, f, precision=prec) if call == "zoom" else S.shift_batched(x, (0.37, -0.61), precision=prec),)
        else:
            lr = np.rint(rng.uniform(0, 255, (B, len(sh), h, w)))
            hr0 = rng.uniform(0, 255, (B, h * f, w * f))
            outs = (S.shift_and_add_batched(lr, sh, f, precision=prec, flags=fl),) if call == "saa" else \
                S.ibp_batched(lr, sh, PSFS[pn](), hr0, f, WALK_ITERS, 0.5, precision=prec, flags=fl)
        torch.cuda.synchronize()
        counts = launches(lib)
        lib.srx_profile_enable(0)
        if want is not None:
            assert S.last_path() == want, (name, S.last_path())
        digest = [hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for t in outs]
        print(f"{name} flags={fl:#x}: path={want} out={' '.join(digest)} launches={' '.join(f'{k}:{v}' for k, v in sorted(counts.items()))}", flush=True)
    return 1 if bad else 0


def planned(prec, sh, psf, h, w, f, flags=0, call="ibp"):
    sh = np.ascontiguousarray(np.asarray(sh, dtype=np.float64))
    k = np.ascontiguousarray(psf)
    eb, shp = 8 if prec == "f64" else 4, sh.ctypes.data_as(_lib._HD)
    if call == "saa":
        return _lib.load().srx_saa_path_for(eb, len(sh), h, w, f, shp, flags).decode()
    return _lib.load().srx_ibp_path_for(eb, len(sh), h, w, h * f, w * f, f, shp, k.ctypes.data_as(_lib._HD), k.shape[0], k.shape[1], flags).decode()


def launches(lib):
    """{kernel name: launches} since srx_profile_enable(1), the kernels that ran only"""
    import ctypes
    out = {}
    for i in range(lib.srx_profile_kernel_count()):
        ms, n = ctypes.c_double(), ctypes.c_long()
        _lib.check(lib.srx_profile_get(i, ctypes.byref(ms), ctypes.byref(n)), "srx_profile_get")
        if n.value:
            out[lib.srx_profile_kernel_name(i).decode()] = n.value
    return out


def flag_cases(plan_only):
    if not plan_only:
        import torch
        from sr_mi355x import api as S
    lib, psf, bad = _lib.load(), PSFS["gauss"](), 0
    print(FLAGS_HEADER)
    for i, (name, call, want, prec, B, f, h, w, sh, base, flag) in enumerate(FLAG_CASES):
        rng = np.random.default_rng(2000 + i)
        lr = np.rint(rng.uniform(0, 255, (B, len(sh), h, w)))
        hr0 = rng.uniform(0, 255, (B, h * f, w * f))
        seen = []
        for fl in (base, base | flag):
            if plan_only:
                got = planned(prec, sh, psf, h, w, f, fl, "saa" if call == "saa" else "ibp")
                print(f"{name} flags={fl:#x}: {got}" + ("" if got == want else f"  (WANTED {want})"))
                bad += got != want
                continue
            lib.srx_profile_enable(1)
            if call == "saa":
                outs = (S.shift_and_add_batched(lr, sh, f, precision=prec, flags=fl),)
            elif call == "ibp_u8":
                outs = S.ibp_u8_batched(lr.astype(np.uint8), sh, psf, hr0, f, 3, 0.5, precision=prec, flags=fl)
            else:
                outs = S.ibp_batched(lr, sh, psf, hr0, f, 3, 0.5, precision=prec, flags=fl)
            torch.cuda.synchronize()
            counts = launches(lib)
            lib.srx_profile_enable(0)
            assert S.last_path() == want, (name, fl, S.last_path())
            digest = [hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for t in outs]
            if fl & L.FLAG_DIAG_V1:  # k_fwd_residual sums the trace with float64 atomics over an item's blocks: the last bits follow their order
                digest[1] = "trace~" + ",".join(f"{v:.10g}" for v in outs[1].cpu().numpy().ravel())
            seen.append((digest, counts))
            print(f"{name} flags={fl:#x}: path={want} out={' '.join(digest)} launches={' '.join(f'{k}:{v}' for k, v in sorted(counts.items()))}", flush=True)
        if not plan_only:
            print(f"{name}: " + ("off == on" if seen[0] == seen[1] else "off != on (" + ", ".join(
                w for w, d in (("bits", seen[0][0] != seen[1][0]), ("launches", seen[0][1] != seen[1][1])) if d) + ")"), flush=True)
    return 1 if bad else 0


def main(argv):
    plan_only = "--plan" in argv
    if "--flags" in argv:
        return flag_cases(plan_only)
    if "--walk" in argv:
        return walk_cases(plan_only)
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
