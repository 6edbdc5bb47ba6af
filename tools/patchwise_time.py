#!/usr/bin/env python3
"""HIP-event times of the patch-wise reconstruction (sr_mi355x/patchwise.py) on the mono_cal_target shape: 5 uint8 frames of 1536 x 2048,
x2, float32, 80 iterations, the default grid (14 x 19 = 266 patches of 128 x 128 LR samples).  The frames are synthetic: one scene through
the library's forward model at shifts up to 0.07 px off the nominal table, so that the field differs from the table and the per-patch
tables take the route real ones would.

Stages, each on its own: gather (srx_patches_gather_u8), the shift field (one estimate_shifts call with B = 266; it ends in a device-to-host
copy, which is inside its time), shift_and_add and ibp of the batch under the one table ("global") and under the per-patch tables ("local"),
blend (srx_patches_blend_f32).  Wholes: reconstruct_patchwise global and local, and session.reconstruct on the same frames (the whole-frame
path, which none of this touches).  One event pair per call, best of --iters calls after --warmup, --rounds rounds in which the forms
alternate; the spread stated is that of the rounds' bests.

gather and blend are bandwidth kernels: their bytes (computed from the shapes, not counted: gather reads and writes P N 128^2 bytes, blend
reads P 256^2 and writes H W float32) over their time, as a share of the rate of a device-to-device copy of a buffer of the blend's size on
the same box, and of the 8 TB/s HBM peak.  Both working sets fit the 256 MB Infinity Cache, so neither is an HBM figure.

Also recorded: the PSNR of the "global" patch-wise image against the whole-frame image (the price of cutting), and the field's statistics.

usage: tools/patchwise_time.py [--iters N] [--warmup N] [--rounds N] [--n-iter N] [--json PATH]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
from sr_mi355x import api, patchwise, session, synth  # noqa: E402

HBM = 8.0e12
H_LR, W_LR, F = 1536, 2048, 2


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


TRUE_OFFSETS = [(0.0, 0.0), (-0.028, 0.066), (-0.010, -0.036), (0.020, 0.045), (0.014, -0.063)]  # off the nominal table by up to 0.07 px


def scene_frames(psf, table):
    """5 uint8 frames of one smooth random scene through the library's own forward model (PSF, sub-pixel shift, decimation) at shifts that
    depart from the nominal table by TRUE_OFFSETS -- as rgb_cal_target's measured table does -- plus N(0, 1) noise, rounded"""
    rng = np.random.default_rng(5)
    small = rng.uniform(0.0, 1.0, (F * H_LR // 8 + 1, F * W_LR // 8 + 1))
    hr = np.kron(small, np.ones((8, 8)))[:F * H_LR, :F * W_LR]
    for _ in range(3):  # three box passes: smooth on the scale of a few samples, structure everywhere
        hr = (hr + np.roll(hr, 3, 0) + np.roll(hr, -3, 0) + np.roll(hr, 3, 1) + np.roll(hr, -3, 1)) / 5.0
    hr = torch.from_numpy(30.0 + 190.0 * (hr - hr.min()) / (hr.max() - hr.min())).to("cuda")
    gen = torch.Generator(device="cuda").manual_seed(6)
    frames = []
    for (sy, sx), (ey, ex) in zip(table, TRUE_OFFSETS):
        clean = api.forward_model_batched(hr[None], psf, (sy + ey, sx + ex), F, precision="f64")[0]
        noisy = clean + torch.randn(clean.shape, generator=gen, device="cuda", dtype=torch.float64)
        frames.append(torch.clamp(torch.round(noisy), 0, 255).to(torch.uint8))
    return frames


def stat(ts):
    return dict(us=float(min(ts)), us_rounds=ts, spread=(max(ts) - min(ts)) / min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-iter", type=int, default=80)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "patchwise_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patchwise_time.py needs a GPU")
    api.set_precision("f32")
    psf = synth.gaussian_psf()
    table = np.asarray([s for _, s in session.IMAGE_SHIFTS], dtype=np.float64)
    frames = scene_frames(psf, table)
    lr = torch.stack(frames)
    grid = patchwise.PatchGrid(H_LR, W_LR, F)
    N, P = len(frames), grid.P
    patches = patchwise.gather(lr, grid)
    field = patchwise.estimate_shift_field(lr, table, grid)
    tables = np.ascontiguousarray(field["used"].reshape(P, N, 2))
    saa = {"global": api.shift_and_add_u8_batched(patches, table, F), "local": api.shift_and_add_u8_batched(patches, tables, F)}
    routes = {}
    hr = {}
    for form, t in (("global", table), ("local", tables)):
        hr[form], _ = api.ibp_u8_batched(patches, t, psf, saa[form].clone(), F, a.n_iter, 0.5)
        routes[form] = api.last_path()
    big = torch.empty((grid.H, grid.W), dtype=torch.float32, device="cuda")
    big2 = torch.empty_like(big)

    calls = {
        "gather_u8": lambda: patchwise.gather(lr, grid),
        "field": lambda: patchwise.estimate_shift_field(lr, table, grid),
        "saa_global": lambda: api.shift_and_add_u8_batched(patches, table, F),
        "saa_local": lambda: api.shift_and_add_u8_batched(patches, tables, F),
        "ibp_global": lambda: api.ibp_u8_batched(patches, table, psf, saa["global"], F, a.n_iter, 0.5, want_errors=False),
        "ibp_local": lambda: api.ibp_u8_batched(patches, tables, psf, saa["local"], F, a.n_iter, 0.5, want_errors=False),
        "blend_f32": lambda: patchwise.blend(hr["local"], grid),
        "d2d_copy_of_one_hr_plane": lambda: big2.copy_(big),
        "reconstruct_patchwise_global": lambda: patchwise.reconstruct_patchwise(frames, table, psf, a.n_iter, F, grid=grid, local=False),
        "reconstruct_patchwise_local": lambda: patchwise.reconstruct_patchwise(frames, table, psf, a.n_iter, F, grid=grid, local=True),
        "session_reconstruct_whole_frame": lambda: session.reconstruct(frames, table, psf, a.n_iter),
    }
    times = {k: [] for k in calls}
    for _ in range(a.rounds):  # the forms alternate inside a round
        for k, fn in calls.items():
            times[k].append(best_us(fn, a.iters, a.warmup))
    out = {k: stat(v) for k, v in times.items()}

    copy_rate = 2.0 * big.numel() * 4 / (out["d2d_copy_of_one_hr_plane"]["us"] * 1e-6)
    g_bytes = 2.0 * P * N * grid.patch_lr ** 2
    b_bytes = float(P) * grid.L_hr ** 2 * 4 + float(grid.H) * grid.W * 4
    for key, nbytes in (("gather_u8", g_bytes), ("blend_f32", b_bytes)):
        rate = nbytes / (out[key]["us"] * 1e-6)
        out[key].update(bytes=nbytes, tb_per_s=rate * 1e-12, share_of_d2d_copy_rate=rate / copy_rate, share_of_hbm_peak=rate / HBM)
    out["d2d_copy_of_one_hr_plane"].update(bytes=2.0 * big.numel() * 4, tb_per_s=copy_rate * 1e-12)

    whole, _ = session.reconstruct(frames, table, psf, a.n_iter)
    glo, _, _ = patchwise.reconstruct_patchwise(frames, table, psf, a.n_iter, F, grid=grid, local=False)
    loc, _, _ = patchwise.reconstruct_patchwise(frames, table, psf, a.n_iter, F, grid=grid, local=True)
    w = whole["SAA_IBP"].cpu().numpy().astype(np.float64)
    cut = {"psnr_db_global_patchwise_vs_whole_frame": synth.psnr(glo["SAA_IBP"].cpu().numpy(), w),
           "psnr_db_local_patchwise_vs_whole_frame": synth.psnr(loc["SAA_IBP"].cpu().numpy(), w),
           "max_abs_global_patchwise_vs_whole_frame": float(np.abs(glo["SAA_IBP"].cpu().numpy() - w).max())}
    true = table + np.asarray(TRUE_OFFSETS)
    fstat = {"status_counts": np.bincount(field["status"].ravel(), minlength=5).tolist(),
             "true_offsets_from_the_table": TRUE_OFFSETS,
             "max_abs_used_minus_table": float(np.abs(field["used"] - table).max()),
             "max_abs_used_minus_true": float(np.abs(field["used"] - true).max()),
             "rms_used_minus_true": float(np.sqrt(np.mean((field["used"] - true) ** 2)))}
    res = dict(device=torch.cuda.get_device_name(0), workload=dict(frames=N, h=H_LR, w=W_LR, factor=F, precision="f32", n_iter=a.n_iter,
               grid=[grid.gy, grid.gx], patches=P, patch_lr=grid.patch_lr, overlap_lr=grid.overlap_lr, margin_hr=grid.margin_hr),
               method=dict(iters=a.iters, warmup=a.warmup, rounds=a.rounds, time="best of iters per round, least of the rounds; spread = (max - min) / min of the rounds' bests"),
               routes=routes, times=out, cut=cut, field=fstat)
    for k, v in out.items():
        extra = f"  {v['tb_per_s']:.2f} TB/s" + (f" = {100 * v['share_of_d2d_copy_rate']:.0f} % of the copy's rate" if "share_of_d2d_copy_rate" in v else "") if "tb_per_s" in v else ""
        print(f"{k:>34}: {v['us'] / 1e3:9.3f} ms (spread {100 * v['spread']:.1f} %){extra}")
    print(f"routes: {routes}; cut: {cut}; field: {fstat}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            json.dump(res, fp, indent=1)


if __name__ == "__main__":
    main()
