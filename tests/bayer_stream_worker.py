"""Worker of tests/test_gpu_bayer_contract.py: tests/stream_contract_worker.py for the entry points of include/srx_bayer.h (a process of its
own for the same reason: the HIP runtime reads DEBUG_CLR_GRAPH_PACKET_CAPTURE once, when it loads, and launches of an instantiated graph
run with it off).

    python bayer_stream_worker.py [case id ...]

runs the cases below through tests/streamcheck.py and prints one JSON line {case id: {"ok": bool, "nodes": {...}, "detail": str}}.  The
first HIP call of the checker that fails, a captured call that returns an error and any exception end the run there: the line then holds
the cases finished so far (plus the one that stopped it, not ok), the exit status is 3 and nothing more is started on the device."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: the graph API is bound to the runtime torch has loaded)
import stream_contract_cases as C  # noqa: E402  (its helpers; its table is not run here)
import streamcheck as SC  # noqa: E402

T, U8 = C.T, torch.uint8
B, H, W, R = 2, 18, 40, 3      # raw frames: H W = 720 = 45 x 16 (the vector kernel), W no multiple of 16: every row has its own cut
HP, WP, D = 21, 37, 1          # HR planes of the merge
PNG_H, PNG_W = 70, 340         # 70 x 1021 scanline bytes: three 32 KB chunks
CASES = {}                     # id -> (make, documented kernel nodes)


def _split(kind):
    def make():
        fn = getattr(T.lib(), "srx_bayer_split_" + kind)
        (x,), samples = C.inputs(C.u8sets((B, H, W), 61) if kind == "u8" else C.fsets((B, H, W), kind, 61, integer=False))
        o = C.out((B, 4, H // 2, W // 2), T.DT.get(kind, U8))
        return SC.Inst(lambda s: fn(T.p(x), B, H, W, T.p(o), C.sp(s)), [x], samples, [o])
    return make


def _mean(prec, shape):
    def make():
        h, w = shape
        (x,), samples = C.inputs(C.u8sets((B, R, h, w), 62))
        o = C.out((B, 4, h // 2, w // 2), T.DT[prec])
        return SC.Inst(lambda s: T.lib().srx_bayer_mean_u8(T.p(x), B, R, h, w, T.EB[prec], T.p(o), C.sp(s)), [x], samples, [o])
    return make


def _merge(entry, prec, gains):
    def make():
        fn = T.fn(entry, prec)
        (x,), samples = C.inputs([t * 1.2 - 20 for t in C.fsets((B, 4, HP, WP), prec, 63, integer=False)])
        o = C.out((B, HP, WP, 3), U8) if entry.endswith("rgb8") else C.out((B, 3, HP, WP), T.DT[prec])
        g, gp = C.hd([1.5, 1.0, 0.75]) if gains else (None, None)   # a host array: read before the call returns, not at the launch
        return SC.Inst(lambda s: fn(T.p(x), B, HP, WP, D, gp, T.p(o), C.sp(s)), [x], samples, [o], host=[g] if gains else [])
    return make


def _rgb_images(k):
    """one compressible image and one random one; sets 1 and 2 swap which item compresses, so lengths[b] changes between capture and launch"""
    rng = np.random.default_rng(201 + k)
    yy, xx = np.mgrid[:PNG_H, :PNG_W]
    smooth = np.stack([(30 + 3 * k + xx // 5 + yy // 2) % 256, (200 - xx // 3 + yy) % 256, (xx + yy) // 4 % 256], axis=-1)
    noise = rng.integers(0, 256, (PNG_H, PNG_W, 3))
    return C.dev(np.stack([smooth, noise] if k == 0 else [noise, smooth]), U8)


def _png():
    def make():
        L = T.lib()
        (x,), samples = C.inputs([_rgb_images(k) for k in range(3)])
        slots, lengths = C.out((B, L.srx_png_file_rgb8_bound(PNG_H, PNG_W)), U8), C.out((B,), torch.int64)
        wt, wp, wn = C.ws(L.srx_png_file_rgb8_scratch_bytes(B, PNG_H, PNG_W))
        return SC.Inst(lambda s: L.srx_png_file_rgb8(T.p(x), B, PNG_H, PNG_W, T.p(slots), T.p(lengths), wp, wn, C.sp(s)), [x], samples,
                       [slots, lengths], wt, written=C._slots)
    return make


for _k in ("u8", "f32", "f64"):
    CASES[f"srx_bayer_split_{_k}-B2_18x40"] = (_split(_k), 1)
for _pr in T.PRECS:
    CASES[f"srx_bayer_mean_u8-{_pr}-R3_18x40"] = (_mean(_pr, (H, W)), 1)
    CASES[f"srx_bayer_mean_u8-{_pr}-R3_18x34"] = (_mean(_pr, (18, 34)), 1)   # H W no multiple of 16: the sample-by-sample kernel
    for _e in ("srx_bayer_merge", "srx_bayer_merge_rgb8"):
        CASES[f"{_e}_{_pr}-B2_21x37_d1-gains"] = (_merge(_e, _pr, True), 1)
        CASES[f"{_e}_{_pr}-B2_21x37_d1-no_gains"] = (_merge(_e, _pr, False), 1)
CASES["srx_png_file_rgb8-B2_70x340"] = (_png(), 5)


def run(only=()):
    lib = T.lib()
    res, stopped = {}, False
    for cid, (make, kernels) in CASES.items():
        if only and cid not in only:
            continue
        try:
            res[cid] = SC.check(make=make, kernels=kernels, copies=0, profile_off=lambda: lib.srx_profile_enable(0))
            stopped = bool(res[cid].pop("stop", False))
        except Exception as e:  # noqa: BLE001  (HipFailure, a torch error after a device fault, a builder's assertion: stop either way)
            res[cid] = {"ok": False, "nodes": {}, "detail": f"{type(e).__name__}: {e}"[:600]}
            stopped = True
        if stopped:
            break
    return res, stopped


if __name__ == "__main__":
    results, stop = run(sys.argv[1:])
    print(json.dumps(results), flush=True)
    sys.exit(3 if stop else 0)
