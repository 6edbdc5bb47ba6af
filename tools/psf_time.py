#!/usr/bin/env python3
"""HIP-event time per call of srx_psf_estimate_{u8,f32} on the reference's calibration stack (30 pinhole frames of 1536 x 2048,
halfwidth 3) and on a 90-frame float32 stack, beside the torch composition a user would write instead on the same device tensors
(frames.view(N, -1).argmax(1), then gather, mean, background, clip and normalise; no host synchronisation either).  One event pair
per call, median of --iters calls after --warmup, the two alternating in the same process.

The call reads every frame once: bytes = N H W sizeof(T), reported over the median time as a fraction of the 8 TB/s HBM peak.  The
uint8 stack is 94 MB and the Infinity Cache 256 MB, so repeated calls on it may be served from the cache and its figure is no HBM
figure; the float32 stacks (377 MB and 1.13 GB) exceed the cache, and the bandwidth to quote is theirs.
Prints one line per workload; --json PATH writes them.

usage: tools/psf_time.py [--iters N] [--warmup N] [--json PATH]
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
from sr_mi355x import _lib, api  # noqa: E402

HBM = 8.0e12
H, W, HALFWIDTH = 1536, 2048, 3
REACH, SIDE = HALFWIDTH + 6, 2 * HALFWIDTH + 1


def median_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def pinhole_stack(N, dtype, seed):
    """N frames of sensor noise (0 .. 9) with one spot of peak 200 .. 240 at a seeded position each"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, 10, (N, H, W), generator=g, device="cuda", dtype=torch.uint8)
    pos = np.random.default_rng(seed).integers(40, [H - 40, W - 40], (N, 2))
    yy, xx = torch.meshgrid(torch.arange(-8, 9, device="cuda"), torch.arange(-8, 9, device="cuda"), indexing="ij")
    for k, (r, c) in enumerate(pos):
        spot = (200 + 4 * (k % 11)) * torch.exp(-(yy.double() ** 2 + xx.double() ** 2) / (2 * 1.5 ** 2))
        x[k, r - 8:r + 9, c - 8:c + 9] += spot.to(torch.uint8)
    return x.to(dtype).contiguous(), pos


class TorchForm:
    """the composition on device tensors; index helpers are made once, outside the timed calls"""

    def __init__(self, N):
        self.n = torch.arange(N, device="cuda")[:, None, None]
        self.span = torch.arange(-REACH, REACH + 1, device="cuda")
        self.edge = torch.from_numpy(np.r_[0:3, SIDE - 3:SIDE]).to("cuda")

    def __call__(self, frames):
        N = frames.shape[0]
        idx = frames.view(N, -1).argmax(1)
        r, c = idx // W, idx % W
        used = ((r >= REACH) & (r + REACH < H) & (c >= REACH) & (c + REACH < W)).to(torch.float64)[:, None, None]
        rr, cc = (r[:, None] + self.span).clamp(0, H - 1), (c[:, None] + self.span).clamp(0, W - 1)
        wins = frames[self.n, rr[:, :, None], cc[:, None, :]].to(torch.float64)
        core = ((wins * used).sum(0) / used.sum())[6:6 + SIDE, 6:6 + SIDE]
        core = (core - core[self.edge][:, self.edge].mean()).clamp_min(0.0)
        return core / core.sum(), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("psf_time.py needs a GPU")
    lib = _lib.load()
    st = api._stream()
    rows = []
    for name, N, dtype, sfx in (("reference stack", 30, torch.uint8, "u8"), ("reference stack", 30, torch.float32, "f32"),
                                ("3 x reference stack", 90, torch.float32, "f32")):
        frames, pos = pinhole_stack(N, dtype, 3)
        eb = frames.element_size()
        n = lib.srx_psf_estimate_workspace_bytes(eb, N, H, W, HALFWIDTH)
        ws = torch.empty(n, dtype=torch.uint8, device="cuda")
        psf = torch.empty((SIDE, SIDE), dtype=torch.float64, device="cuda")
        info = torch.empty((N, 3), dtype=torch.int32, device="cuda")
        fn = getattr(lib, f"srx_psf_estimate_{sfx}")

        def call():
            _lib.check(fn(api._p(frames), N, H, W, HALFWIDTH, api._p(psf), api._p(info), api._p(ws), ctypes.c_size_t(n), st), "srx_psf_estimate")

        form = TorchForm(N)
        note = ""
        try:
            ref_psf, ref_idx = form(frames)
        except RuntimeError as e:  # an argmax this dtype does not have: the user converts first, inside the timed call
            note = f"torch argmax refused {dtype} ({str(e).splitlines()[0]}): composition on frames.float()"
            inner = form
            form = lambda f: inner(f.float())  # noqa: E731
            ref_psf, ref_idx = form(frames)
        call()
        torch.cuda.synchronize()
        peaks = info.cpu().numpy()
        assert np.array_equal(peaks[:, 0].astype(np.int64) * W + peaks[:, 1], ref_idx.cpu().numpy()) and peaks[:, 2].all()
        assert np.array_equal(peaks[:, :2], pos)
        diff = float((psf - ref_psf).abs().max())
        assert diff < 1e-12, diff
        t_lib = t_torch = None
        for _ in range(2):  # alternate the two; keep the better median of each
            tl, tt = median_us(call, a.iters, a.warmup), median_us(lambda: form(frames), a.iters, a.warmup)
            t_lib, t_torch = (tl if t_lib is None else min(t_lib, tl)), (tt if t_torch is None else min(t_torch, tt))
        nbytes = float(N) * H * W * eb
        rows.append(dict(case=name, dtype=sfx, N=N, H=H, W=W, bytes=nbytes, exceeds_infinity_cache=nbytes > 256 * 2 ** 20, us_call=t_lib,
                         tb_per_s=nbytes / t_lib * 1e-6, fraction_of_hbm_peak=nbytes / HBM / (t_lib * 1e-6), us_torch=t_torch,
                         torch_over_call=t_torch / t_lib, max_abs_diff_vs_torch=diff, note=note))
        del frames, ws, form
        torch.cuda.empty_cache()
    for x in rows:
        print(f"{x['case']:>20} {x['dtype']:>3} N={x['N']:2d} {x['bytes'] / 1e6:7.1f} MB{'' if x['exceeds_infinity_cache'] else ' (fits the Infinity Cache)'}: "
              f"{x['us_call']:8.1f} us per call = {x['tb_per_s']:5.2f} TB/s = {100 * x['fraction_of_hbm_peak']:5.1f} % of 8 TB/s; torch composition "
              f"{x['us_torch']:8.1f} us ({x['torch_over_call']:.2f} x the call)  {x['note']}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak=HBM, iters=a.iters, warmup=a.warmup, rows=rows), f, indent=1)
    slower = [x for x in rows if x["us_call"] > x["us_torch"]]
    if slower:
        raise SystemExit(f"the library call is slower than the torch composition on {[(x['dtype'], x['N']) for x in slower]}")


if __name__ == "__main__":
    main()
