#!/usr/bin/env python3
"""HIP-event time per call of srx_ssim_{f32,f64} on one and eight 3072 x 4096 pairs (the cal-target HR frame), uniform 7 x 7 and
Gaussian sigma 1.5 (11 x 11) windows, with and without the map, next to srx_pair_moments_* on the same pair (which reads the same
bytes).  The roofline fraction is the least time the reads (2 B H W sizeof(T), plus the map when written) take at 8 TB/s over the
measured time.  Prints one line per case and, with --json PATH, writes them all.

usage: tools/ssim_time.py [--iters N] [--warmup N] [--json PATH]
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
from sr_mi355x import _lib, api, metrics  # noqa: E402

HBM = 8.0e12
H, W = 3072, 4096


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_time.py needs a GPU")
    lib = _lib.load()
    st = api._stream()
    rows = []
    g = torch.Generator(device="cuda").manual_seed(7)
    for B in (1, 8):
        base = torch.randint(0, 256, (B, H, W), generator=g, device="cuda", dtype=torch.int32).double()
        other = (0.8 * base + torch.randint(0, 40, (B, H, W), generator=g, device="cuda", dtype=torch.int32).double()).round()
        n = lib.srx_metrics_workspace_bytes(B, H, W, 1)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        wp, wn = api._p(ws), ctypes.c_size_t(n)
        mom = torch.empty((B, 7), dtype=torch.float64, device="cuda")
        mssim = torch.empty(B, dtype=torch.float64, device="cuda")
        for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
            r, t = base.to(dt), other.to(dt)
            eb = r.element_size()
            smap = torch.empty((B, H, W), dtype=dt, device="cuda")
            pm = getattr(lib, f"srx_pair_moments_{prec}")
            t_pm = timed(lambda: pm(api._p(r), api._p(t), B, H, W, 0, api._p(mom), wp, wn, st), a.iters, a.warmup)
            rd = 2.0 * B * H * W * eb
            rows.append(dict(kernel=f"pair_moments_{prec}", B=B, us=t_pm, bytes=rd, roofline=rd / HBM / (t_pm * 1e-6)))
            fn = getattr(lib, f"srx_ssim_{prec}")
            for win, gauss in (("uniform7", False), ("gauss11", True)):
                rad, taps, _ = metrics.ssim_params((H, W), np.uint8, gaussian_weights=gauss)
                tp = taps.ctypes.data_as(_lib._HD)
                for with_map in (False, True):
                    mp = api._p(smap) if with_map else None
                    us = timed(lambda: fn(api._p(r), api._p(t), B, H, W, 0, rad, tp, 1, 255.0, 0.01, 0.03, None, api._p(mssim), mp, wp, wn, st),
                               a.iters, a.warmup)
                    by = rd + (B * H * W * eb if with_map else 0.0)
                    rows.append(dict(kernel=f"ssim_{prec}", window=win, map=with_map, B=B, us=us, bytes=by, roofline=by / HBM / (us * 1e-6),
                                     vs_pair_moments=us / t_pm))
            del r, t, smap
        del base, other, ws
        torch.cuda.empty_cache()
    for x in rows:
        extra = f" {x['window']:>8} map={int(x['map'])} x{x['vs_pair_moments']:.2f} of pair_moments" if "window" in x else ""
        print(f"{x['kernel']:>16} B={x['B']} {x['us']:9.1f} us  {x['bytes'] / x['us'] * 1e-6:5.2f} TB/s  roofline {100 * x['roofline']:5.1f} %{extra}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), H=H, W=W, hbm_peak=HBM, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
