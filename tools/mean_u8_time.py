#!/usr/bin/env python3
"""HIP-event time per call of api.mean_u8 (srx_mean_u8) beside the composition the session ran before it on the same uint8 device
stack, both giving float64 (session.LOADER_PRECISION):

    rep mean of the red planes (f = 2):  per item, per rep  u8_to_float -> extract_red;  mean_frames of the reps   (load_rgb_cal_combo)
    frame mean (f = 1):                  mean_frames_batched(u8_to_float(stack))                                   (reconstruct*)

One event pair per call, median of --iters calls after --warmup; the two forms alternate in one process for --rounds rounds, and the
spread recorded is that of the rounds' medians.  `faster_beyond_spread`: the composition's fastest round is slower than mean_u8's slowest.

Bytes: what the shape implies -- the rows read whole, B R ceil((H - py) / f) W, plus the output B h w 8 -- over the median time, as a
share of the 8 TB/s HBM peak.  These are computed from the shapes, not counted.  A stack that fits the 256 MB Infinity Cache (one
rgb_cal_target combo is 63 MB) may be served from it on repeated calls, so its figure is no HBM figure; the `large` rows (no composition
beside them: its float64 copy would be 8 x the stack) exceed the cache and theirs is the bandwidth to quote.

Loader leg: a seeded 20-file rgb_cal_target combo of the reference's size (4 corners x 5 reps of 1536 x 2048) is written to a temporary
directory; a host clock around session.load_rgb_cal_combo ending in a device synchronise, keep_u8 False and True alternating; the PNG
decode, common to both, is timed on its own.  The uploaded bytes are computed from the shapes.

usage: tools/mean_u8_time.py [--iters N] [--warmup N] [--rounds N] [--json PATH] [--no-loader]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
from sr_mi355x import api, session  # noqa: E402

HBM = 8.0e12
CACHE = 256 * 2 ** 20
PREC = session.LOADER_PRECISION

CASES = (
    # name, B, R, H, W, f, with the composition beside it
    ("rgb_cal_target combo", 4, 5, 1536, 2048, 2, True),
    ("mono_cal_target frame mean", 1, 5, 1536, 2048, 1, True),
    ("barcode session reps", 8, 4, 768, 1024, 1, True),
    ("large, f = 2", 48, 5, 1536, 2048, 2, False),
    ("large, f = 1", 24, 5, 1536, 2048, 1, False),
)


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


def composition(x, f):
    with api.precision_override(PREC):
        if f == 1:
            return api.mean_frames_batched(api.u8_to_float(x, PREC))
        return [api.mean_frames([api.extract_red(api.u8_to_float(x[b, r], PREC)) for r in range(x.shape[1])]) for b in range(x.shape[0])]  # a list, as the loader keeps it


def call_rows(a):
    rows = []
    for name, B, R, H, W, f, beside in CASES:
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.randint(0, 256, (B, R, H, W), generator=g, device="cuda", dtype=torch.uint8)
        call = lambda: api.mean_u8(x, f, precision=PREC)  # noqa: E731
        h, w = -(-H // f), -(-W // f)
        read, written = float(B) * R * h * W, float(B) * h * w * 8
        row = dict(case=name, B=B, R=R, H=H, W=W, f=f, stack_bytes=float(B) * R * H * W, bytes_read=read, bytes_written=written,
                   fits_infinity_cache=read + written <= CACHE)
        if beside:
            ref = composition(x, f)
            assert torch.equal(call(), ref if isinstance(ref, torch.Tensor) else torch.stack(ref))
        t_call, t_comp = [], []
        for _ in range(a.rounds):
            t_call.append(median_us(call, a.iters, a.warmup))
            if beside:
                t_comp.append(median_us(lambda: composition(x, f), a.iters, a.warmup))
        us = float(np.median(t_call))
        row.update(us_mean_u8=us, us_mean_u8_rounds=t_call, spread_mean_u8=(max(t_call) - min(t_call)) / min(t_call),
                   tb_per_s=(read + written) / us * 1e-6, share_of_hbm_peak=(read + written) / HBM / (us * 1e-6))
        if beside:
            uc = float(np.median(t_comp))
            row.update(us_composition=uc, us_composition_rounds=t_comp, spread_composition=(max(t_comp) - min(t_comp)) / min(t_comp),
                       composition_over_mean_u8=uc / us, faster_beyond_spread=min(t_comp) > max(t_call))
        rows.append(row)
        del x
        torch.cuda.empty_cache()
    return rows


def loader_leg(rounds):
    H, W, corners, reps = 1536, 2048, 4, 5
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 110 + 70 * np.sin(yy / 37.0) * np.cos(xx / 53.0)
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for c in range(corners):
            for r in range(reps):
                fr = np.clip(np.roll(base, (c % 2, c // 2), axis=(0, 1)) + rng.normal(0, 2.0, (H, W)), 0, 255).astype(np.uint8)
                paths.append(os.path.join(d, f"corner{c}_rep{r:02d}.png"))
                session.write_png_u8(paths[-1], fr)
        meta = {"expected_shifts": {lab: {"dy_px": dy, "dx_px": dx} for lab, (dy, dx) in zip(session.CORNER_ORDER, ((1, -1), (1, 1), (-1, -1), (-1, 1)))}}
        with open(os.path.join(d, "metadata.json"), "w") as fp:
            json.dump(meta, fp)
        f0, _ = session.load_rgb_cal_combo(d)
        f1, _ = session.load_rgb_cal_combo(d, keep_u8=True)
        assert all(torch.equal(a, b) for a, b in zip(f0, f1))
        t = {False: [], True: [], "decode": []}
        for _ in range(rounds):
            t0 = time.perf_counter()
            session._decode_many(paths)
            t["decode"].append((time.perf_counter() - t0) * 1e3)
            for keep in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                session.load_rgb_cal_combo(d, keep_u8=keep)
                torch.cuda.synchronize()
                t[keep].append((time.perf_counter() - t0) * 1e3)
    n = corners * reps * H * W
    return dict(files=corners * reps, H=H, W=W, rounds=rounds, ms_png_decode=float(np.median(t["decode"])), ms_png_decode_rounds=t["decode"],
                ms_load_float64=float(np.median(t[False])), ms_load_float64_rounds=t[False], ms_load_keep_u8=float(np.median(t[True])),
                ms_load_keep_u8_rounds=t[True], float64_over_keep_u8=float(np.median(t[False]) / np.median(t[True])),
                computed_device_bytes_float64_frames=float(n) * 8, computed_uploaded_bytes_keep_u8=float(n),
                note="float64 path: every file goes up as bytes and is converted to a float64 frame on the device (8 bytes per sample written "
                     "and read back); keep_u8: the bytes are all there is.  Byte counts computed from the shapes.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--no-loader", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mean_u8_time.py needs a GPU")
    rows = call_rows(a)
    for x in rows:
        line = (f"{x['case']:>28} B={x['B']:2d} R={x['R']} {x['H']}x{x['W']} f={x['f']}: {x['us_mean_u8']:8.1f} us (spread {100 * x['spread_mean_u8']:.1f} %) = "
                f"{x['tb_per_s']:5.2f} TB/s = {100 * x['share_of_hbm_peak']:5.1f} % of 8 TB/s{' (fits the Infinity Cache)' if x['fits_infinity_cache'] else ''}")
        if "us_composition" in x:
            line += (f"; composition {x['us_composition']:8.1f} us (spread {100 * x['spread_composition']:.1f} %) = {x['composition_over_mean_u8']:.1f} x"
                     f"{'' if x['faster_beyond_spread'] else '  NOT beyond the spread'}")
        print(line)
    loader = None if a.no_loader else loader_leg(5)
    if loader:
        print(f"load_rgb_cal_combo, 20 files of 1536 x 2048: float64 {loader['ms_load_float64']:.1f} ms, keep_u8 {loader['ms_load_keep_u8']:.1f} ms "
              f"({loader['float64_over_keep_u8']:.2f} x), of which PNG decode {loader['ms_png_decode']:.1f} ms in both")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak=HBM, infinity_cache_bytes=CACHE, precision=PREC, iters=a.iters, warmup=a.warmup,
                           rounds=a.rounds, rows=rows, loader=loader), f, indent=1)
    slow = [x["case"] for x in rows if "us_composition" in x and not x["faster_beyond_spread"]]
    if slow:
        raise SystemExit(f"mean_u8 is not faster than the composition beyond the spread on {slow}")


if __name__ == "__main__":
    main()
