#!/usr/bin/env python3
"""HIP-event time per call of srx_register_{f32,f64} on session-shaped stacks: mono_cal_target (N = 5 frames of 1536 x 2048 LR) and
rgb_cal_target (N = 4 rep-averaged red planes of 1536 x 2048), search 2, border 8, 10 iterations.  Frames are a smooth random scene
shifted on the device by the jittered +-0.5 px table.  Three calls per case: as used (tol 1e-4: frames stop once converged), all
10 iterations forced (tol 0) and none (n_iter 0: prefilter + coarse search + score pass).  The Gauss-Newton pass reads the moving
frame's spline coefficients and the reference once per iteration (2 sizeof(T) B/px over the crop of every moving frame); its HBM
fraction is that byte count at 8 TB/s over the measured (tol 0 - n_iter 0) / 10.  Prints one line per case; --json PATH writes them.

usage: tools/register_time.py [--iters N] [--warmup N] [--json PATH]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
from sr_mi355x import _lib, api, synth  # noqa: E402

HBM = 8.0e12
H, W = 1536, 2048
SEARCH, BORDER, N_ITER = 2, 8, 10


def timed(fn, iters, warmup):
    for _ in range(warmup):
        _lib.check(fn(), "warmup")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        _lib.check(fn(), "timed")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us per call


def scene(prec):
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((1, 1, H + 64, W + 64), generator=g, device="cuda", dtype=torch.float64)
    k = torch.ones((1, 1, 9, 9), device="cuda", dtype=torch.float64) / 81.0
    x = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, k), k)[0, 0]
    x = (x - x.min()) / (x.max() - x.min()) * 255.0
    return x[:H, :W].contiguous().to(api._TORCH_DT[prec])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("register_time.py needs a GPU")
    lib = _lib.load()
    st = api._stream()
    rows = []
    nom5 = np.asarray(synth.NOMINAL_5)
    jit = np.random.default_rng(5).uniform(-0.1, 0.1, nom5.shape)
    jit[0] = 0.0
    for name, table, prec in (("mono_cal_target", nom5, "f32"), ("rgb_cal_target", nom5[1:], "f32"), ("mono_cal_target", nom5, "f64")):
        N = len(table)
        base = scene(prec)
        frames = torch.stack([api.shift_batched(base[None], s, precision=prec)[0] for s in (table + jit[:N])])[None].contiguous()
        eb = frames.element_size()
        n = lib.srx_register_workspace_bytes(eb, 1, N, H, W, SEARCH)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        shifts = torch.empty((1, N, 2), dtype=torch.float64, device="cuda")
        score = torch.empty((1, N), dtype=torch.float64, device="cuda")
        status = torch.empty((1, N), dtype=torch.int32, device="cuda")
        init = np.ascontiguousarray(table, dtype=np.float64)
        fn = getattr(lib, f"srx_register_{prec}")

        def call(n_iter, tol):
            return fn(api._p(frames), 1, N, H, W, 0, init.ctypes.data_as(_lib._HD), SEARCH, BORDER, n_iter, tol, api._p(shifts), api._p(score),
                      api._p(status), api._p(ws), ctypes.c_size_t(n), st)

        t_used = timed(lambda: call(N_ITER, 1e-4), a.iters, a.warmup)
        t_full = timed(lambda: call(N_ITER, 0.0), a.iters, a.warmup)
        t_none = timed(lambda: call(0, 1e-4), a.iters, a.warmup)
        m = BORDER + SEARCH + 2
        per_iter_bytes = (N - 1) * (H - 2 * m) * (W - 2 * m) * 2.0 * eb
        t_iter = (t_full - t_none) / N_ITER
        _lib.check(call(N_ITER, 1e-4), "check")
        rows.append(dict(case=name, precision=prec, N=N, H=H, W=W, us_used=t_used, us_all_iters=t_full, us_no_iters=t_none, us_per_iter=t_iter,
                         bytes_per_iter=per_iter_bytes, iter_roofline=per_iter_bytes / HBM / (t_iter * 1e-6),
                         status=status.cpu().numpy().tolist()[0], max_err=float(np.abs(shifts.cpu().numpy()[0] - (table + jit[:N] - table[0] - jit[0])).max())))
        del frames, ws, base
        torch.cuda.empty_cache()
    for x in rows:
        print(f"{x['case']:>16} {x['precision']} N={x['N']} {x['H']}x{x['W']}: {x['us_used']:7.1f} us as used, {x['us_all_iters']:7.1f} us with all "
              f"{N_ITER} iterations, {x['us_no_iters']:6.1f} us without; {x['us_per_iter']:5.1f} us/iteration = "
              f"{x['bytes_per_iter'] / x['us_per_iter'] * 1e-6:4.2f} TB/s, roofline {100 * x['iter_roofline']:4.1f} %; status {x['status']} "
              f"max|err| {x['max_err']:.4f} px")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak=HBM, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
