#!/usr/bin/env python3
"""HIP-event times of the colour entry points (include/srx_bayer.h) beside what they replace, both timed in the same run on the same
device buffers, alternating:

    srx_bayer_mean_u8   one rgb_cal_target combo (4 corners x 5 reps of 1536 x 2048), float32 and float64 planes, against srx_mean_u8 x 4
    srx_bayer_split_u8  a 16-frame barcode session (16 frames of 1536 x 2048), against srx_decimate_u8 x 4
    srx_bayer_merge_rgb8_f32, srx_png_file_rgb8 at 1536 x 2048 x 3: the bytes the call moves (computed from the shapes) over its time,
                        beside the rate of a device-to-device copy of as many bytes (read + written) measured here
    the colour reconstruction of one combo (session.reconstruct_colour: four planes as one batch) against the red-only one
                        (session.reconstruct), host clock around calls that end in a device synchronise

One event pair around each call; a round is the best of --iters calls after --warmup; --rounds rounds, the median of the rounds' bests is
the figure and (max - min) / min of them the spread.  Bytes are what the shapes imply, not counted.

usage: tools/bayer_time.py [--iters N] [--warmup N] [--rounds N] [--json PATH] [--recon-iters N]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
from sr_mi355x import api, session, synth  # noqa: E402

H, W = 1536, 2048
PLANES = [(p >> 1, p & 1) for p in range(4)]


def best_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(min(a.elapsed_time(b) for a, b in ev)) * 1e3


def rounds_of(fns, a):
    """the callables alternate within every round -> per callable (median of the rounds' bests, the bests, the spread)"""
    t = [[] for _ in fns]
    for _ in range(a.rounds):
        for k, fn in enumerate(fns):
            t[k].append(best_us(fn, a.iters, a.warmup))
    return [(float(np.median(x)), x, (max(x) - min(x)) / min(x)) for x in t]


def pair_row(name, one, four, nbytes_one, a):
    (u1, r1, s1), (u4, r4, s4) = rounds_of([one, four], a)
    return dict(case=name, us_one_call=u1, us_one_call_rounds=r1, spread_one_call=s1, us_four_calls=u4, us_four_calls_rounds=r4,
                spread_four_calls=s4, four_calls_over_one=u4 / u1, one_call_slower_beyond_spread=min(r1) > max(r4),
                bytes_one_call=nbytes_one, tb_per_s_one_call=nbytes_one / u1 * 1e-6)


def rate_row(name, fn, nbytes, a):
    """a call beside a device-to-device copy that moves as many bytes (half read, half written)"""
    src = torch.empty(int(nbytes) // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    (u, r, s), (uc, rc, sc) = rounds_of([fn, lambda: dst.copy_(src)], a)
    return dict(case=name, us=u, us_rounds=r, spread=s, bytes_moved=nbytes, tb_per_s=nbytes / u * 1e-6, us_copy_of_as_many_bytes=uc,
                us_copy_rounds=rc, spread_copy=sc, tb_per_s_copy=nbytes / uc * 1e-6, share_of_copy_rate=uc / u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--recon-iters", type=int, default=session.IBP_ITERATIONS["rgb_cal_target"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bayer_time.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(7)
    rows = []

    # ---- the rep mean of one combo
    combo = torch.randint(0, 256, (4, 5, H, W), generator=g, device="cuda", dtype=torch.uint8)
    for prec, eb in (("f32", 4), ("f64", 8)):
        one = lambda: api.bayer_mean_u8(combo, precision=prec)  # noqa: E731
        four = lambda: [api.mean_u8(combo, 2, py, px, precision=prec) for py, px in PLANES]  # noqa: E731
        assert all(torch.equal(one()[:, p], x) for p, x in enumerate(four()))
        rows.append(pair_row(f"srx_bayer_mean_u8 {prec}, 4 x 5 x {H} x {W}, against srx_mean_u8 x 4", one, four, float(combo.numel()) * (1 + eb / 5), a))

    # ---- the split of a barcode session
    frames = torch.randint(0, 256, (16, H, W), generator=g, device="cuda", dtype=torch.uint8)
    one = lambda: api.bayer_split(frames)  # noqa: E731
    four = lambda: [api.decimate_u8(frames, 2, py, px) for py, px in PLANES]  # noqa: E731
    assert all(torch.equal(one()[:, p], x) for p, x in enumerate(four()))
    rows.append(pair_row(f"srx_bayer_split_u8, 16 x {H} x {W}, against srx_decimate_u8 x 4", one, four, 2.0 * frames.numel(), a))

    # ---- merge and the RGB file at the reference's HR size
    with api.precision_override("f32"):
        planes = torch.rand((1, 4, H, W), generator=g, device="cuda", dtype=torch.float32) * 255
        rows.append(rate_row(f"srx_bayer_merge_rgb8_f32, {H} x {W} x 3", lambda: api.bayer_merge(planes, 2, (1.5, 1.0, 0.75), rgb8=True),
                             float(H * W) * (4 * 4 + 3), a))
        rgb = api.bayer_merge(planes, 2, None, rgb8=True)
    smooth = (torch.arange(H * W * 3, device="cuda").reshape(1, H, W, 3) // 97 % 256).to(torch.uint8)  # compressible, like a reconstruction
    for name, img in (("noise", rgb), ("smooth", smooth)):
        _, lengths = api.png_file_rgb8(img)
        row = rate_row(f"srx_png_file_rgb8, {H} x {W} x 3, {name}", lambda: api.png_file_rgb8(img), float(H * W * 3) + float(lengths[0]), a)
        row["file_bytes"] = int(lengths[0])
        rows.append(row)

    # ---- the colour reconstruction of one combo against the red-only one
    recon = []
    psf, shifts = synth.gaussian_psf(), np.asarray(synth.NOMINAL_4, dtype=np.float64)
    for prec in ("f32", "f64"):
        with api.precision_override(prec):
            pf = list(api.bayer_mean_u8(combo, precision=session.LOADER_PRECISION))   # 4 frames of [4, h, w]
            red = [f[0] for f in pf]

            def clock(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3

            t_red, t_col = [], []
            for k in range(a.rounds + 1):   # the first round is the warm-up
                tr = clock(lambda: session.reconstruct(red, shifts, psf, a.recon_iters))
                tc = clock(lambda: session.reconstruct_colour(pf, shifts, psf, a.recon_iters))
                if k:
                    t_red.append(tr)
                    t_col.append(tc)
            recon.append(dict(precision=prec, n_iter=a.recon_iters, lr_plane=[H // 2, W // 2], ms_red_only=float(np.median(t_red)), ms_red_only_rounds=t_red,
                              ms_colour=float(np.median(t_col)), ms_colour_rounds=t_col, colour_over_red=float(np.median(t_col) / np.median(t_red))))

    for x in rows:
        if "us_four_calls" in x:
            print(f"{x['case']}: {x['us_one_call']:.1f} us (spread {100 * x['spread_one_call']:.1f} %), four calls {x['us_four_calls']:.1f} us "
                  f"(spread {100 * x['spread_four_calls']:.1f} %) = {x['four_calls_over_one']:.2f} x; {x['tb_per_s_one_call']:.2f} TB/s")
        else:
            print(f"{x['case']}: {x['us']:.1f} us (spread {100 * x['spread']:.1f} %) = {x['tb_per_s']:.2f} TB/s; a copy of as many bytes "
                  f"{x['us_copy_of_as_many_bytes']:.1f} us = {x['tb_per_s_copy']:.2f} TB/s; {100 * x['share_of_copy_rate']:.0f} % of the copy's rate")
    for x in recon:
        print(f"reconstruction of one combo, {x['precision']}, {x['n_iter']} iterations: red only {x['ms_red_only']:.1f} ms, colour {x['ms_colour']:.1f} ms "
              f"= {x['colour_over_red']:.2f} x")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rounds=a.rounds, rows=rows, reconstruction=recon), f, indent=1)


if __name__ == "__main__":
    main()
