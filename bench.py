#!/usr/bin/env python3
"""bench.py -- HR megapixels/s of the SR hot path (SAA + IBP) on N MI355X of one node.

A "step" = one complete reconstruction (shift_and_add + ibp(n_iter)) of one batch of synthetic
patches, with every input already resident in HBM.  The workload is BASELINE.json configs[1] as
SURVEY.md section 8d grounds it (C2): x4 upscale, 64x64 LR patches -> 256x256 HR, N=16 frames at
all 4x4 sub-pixel phases (fractional HR shifts), 7x7 Gaussian PSF, 80 IBP iterations, step 0.5,
B=1024 patches per GPU.  Patches are independent work items: ranks own disjoint patches, no
collective on the data path ("scaling": "weak"); torch.distributed is used only for the barrier
and the max-over-ranks time.

    python bench.py --gpus 1 --steps 3 --warmup 1
    python -m torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8 --steps K --warmup W

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps, writes the last
step's outputs if --dump-outputs DIR is given, and prints the line; `roofline`, `kernels`,
`secondary` and `cpu_baseline` are then empty.  With --full it also measures
  roofline     : dominant kernel, duration measured live with HIP events on the launch stream
  secondary    : the f64 and c3 legs, the files-to-files session leg, SAA alone, host buffers (c2, N = 1)
  cpu_baseline : the CPU oracle (oracle/, a port of the reference's algorithm) timed on this
                 host's cores on a bounded sample of the same workload -- a reported baseline only.

    python bench.py --gpus 1 --steps 20 --warmup 5 --full
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs bench_outputs
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s achievable)
DUMP_BYTES = {"hr": 56 << 20, "errors": 6 << 20}  # --dump-outputs: at most 62 MiB in all, index files included
DUMP_SEED = 459


def make_inputs(S, synth, B, f, lr_hw, shifts, psf, n_unique, prec, seed_base):
    """Synthetic 'DIV2K-shaped' patches: truth images from synth.truth_image, LR frames through the
    product's own forward model + sensor noise (sigma 1 DN), rounded and clipped to the uint8 range."""
    h, w = lr_hw
    H, W = h * f, w * f
    truths = np.stack([synth.truth_image(H, W, seed=seed_base + i) for i in range(n_unique)])
    tt = torch.from_numpy(truths).cuda()
    frames = torch.stack([S.forward_model_batched(tt, psf, s, f, precision=prec) for s in shifts], dim=1)  # [U,N,h,w]
    reps = (B + n_unique - 1) // n_unique
    lr = frames.repeat(reps, 1, 1, 1)[:B].contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(synth.SEED_NOISE + seed_base)
    lr = torch.clamp(torch.round(lr + torch.randn(lr.shape, generator=gen, device="cuda", dtype=lr.dtype)), 0, 255)
    return lr.contiguous(), truths


def kernel_model_bytes(name, B, N, h, w, f, eb, n_iter):
    """Algorithmic (minimum) HBM bytes of ONE launch of a fused-path kernel at these shapes."""
    H, W = h * f, w * f
    hw, pad, lrn = B * H * W * eb, B * (H + 24) * (W + 24) * eb, B * N * h * w * eb
    return {
        "k_blur_pad": 2 * hw,                   # read hr, write the blurred plane (its pad is applied by the tile loaders)
        "k_prefilter_axis0": 2 * pad,           # read + write the padded plane
        "k_prefilter_axis1": 2 * pad,
        "k_fwd_residual": pad + 2 * lrn,        # read coefficients + LR frames, write residuals
        "k_back_gather": lrn + pad,             # read residuals, write padded gather
        "k_blurT_update": pad + 2 * hw,         # read padded coefficients + hr, write hr
        "k_fwd_tile": pad + 2 * lrn,            # read padded blur + LR frames, write residuals
        "k_bwd_tile": lrn + 2 * hw,             # read residuals + hr, write hr
        "k_fwd_mosaic": hw + 2 * B * (H + 27) * (W + 27) * eb,   # read blurred plane (or hr) + LR mosaic, write G
        "k_bwd_mosaic": B * (H + 27) * (W + 27) * eb + 2 * hw,   # read G + hr, write hr
        # one launch = all n_iter iterations of a patch: SURVEY 8d's per-iteration bytes (read + write hr, read the LR samples)
        "k_ibp_patch": n_iter * (2 * hw + lrn),
        "k_ibp_ztile": 2 * hw + lrn,            # one launch = one iteration
        "k_ibp_dtile": 2 * hw + lrn,
        "k_ibp_ctile": 2 * hw + lrn,
        "k_ibp_afwd": 2 * hw + lrn,             # read hr + the LR mosaic, write G
        "k_ibp_abwd": 3 * hw,                   # read G + hr, write hr
        "k_ibp_sv": 3 * hw,                     # read G' + hr, write hr (and Yv: the next launch's input, counted there)
        "k_ibp_sh": hw + lrn + hw,              # read Yv + the LR mosaic, write G'
        "k_ibp_bfwd": hw + 2 * lrn,             # read hr + the LR frames, write the residuals
        "k_ibp_bbwd": lrn + 2 * hw,             # read the residuals + hr, write hr
    }.get(name)


def workload(synth, name, batch, iters):
    """(f, lr_hw, shifts, psf, B, n_iter, description) of a named workload."""
    if name == "c2":
        return (4, (64, 64), synth.phase_shifts(4), synth.gaussian_psf(), batch or 1024, iters or 80,
                "C2: x4 multi-frame SR of 64x64 LR patches -> 256x256 HR, N=16 frames (all 4x4 sub-pixel phases), "
                "7x7 Gaussian PSF, shift_and_add + ibp(80 it, step 0.5)")
    if name == "c2_measured":  # the same patches with a PSF that is not rank 1 (a 5 x 5 core like the reference's load_measured_psf output)
        return (4, (64, 64), synth.phase_shifts(4), synth.asymmetric_psf(), batch or 1024, iters or 80,
                "C2, --psf measured: x4 multi-frame SR of 64x64 LR patches -> 256x256 HR, N=16 frames (all 4x4 sub-pixel phases), "
                "asymmetric (non-separable) 7x7 PSF, shift_and_add + ibp(80 it, step 0.5)")
    if name == "c3_mono":  # mono_cal_target/run_sr.py:50-66: 5 frames, nominal +-0.5 px, f=2, 80 iterations
        return (2, (1536, 2048), synth.NOMINAL_5, synth.gaussian_psf(), batch or 1, iters or 80,
                "C3-mono: the reference's mono_cal_target shape, 1536x2048 LR -> 3072x4096, N=5 nominal shifts, Gaussian PSF")
    if name == "c3_mono_measured":  # the same frames with --psf measured (mono_cal_target/run_sr.py:114-152, 350-355): a PSF that is not rank 1
        return (2, (1536, 2048), synth.NOMINAL_5, synth.asymmetric_psf(), batch or 1, iters or 80,
                "C3-mono, --psf measured: 1536x2048 LR -> 3072x4096, N=5 nominal shifts, asymmetric (non-separable) 7x7 PSF")
    if name == "c3_rgb":   # rgb_cal_target/run_sr.py:49-63, 340-373: 4 frames, measured shifts, f=2, 50 iterations, --psf gaussian (its default)
        return (2, (768, 1024), synth.MEASURED_4, synth.gaussian_psf(), batch or 1, iters or 50,
                "C3-rgb: the reference's rgb_cal_target shape and defaults, 768x1024 LR -> 1536x2048, N=4 measured shifts, Gaussian PSF")
    if name == "c3_rgb_measured":  # the same with --psf measured (rgb_cal_target/run_sr.py:128-166): a PSF that is not rank 1
        return (2, (768, 1024), synth.MEASURED_4, synth.asymmetric_psf(), batch or 1, iters or 50,
                "C3-rgb, --psf measured: 768x1024 LR -> 1536x2048, N=4 measured shifts, asymmetric (non-separable) 7x7 PSF")
    if name == "c3_f4":    # "plus f=4 variant 768x1024 -> 3072x4096"
        return (4, (768, 1024), synth.phase_shifts(4), synth.gaussian_psf(), batch or 1, iters or 80,
                "C3-f4: 768x1024 LR -> 3072x4096 at x4, N=16 frames (all 4x4 sub-pixel phases), Gaussian PSF")
    if name == "c3_f4_measured":  # ... with a PSF that is not rank 1 (the 7 x 7 form of the window kernel)
        return (4, (768, 1024), synth.phase_shifts(4), synth.asymmetric_psf(), batch or 1, iters or 80,
                "C3-f4, --psf measured: 768x1024 LR -> 3072x4096 at x4, N=16 frames (all sub-pixel phases), asymmetric (non-separable) 7x7 PSF")
    if name == "c3_f4_float":  # the same with frames that are not 8-bit integers (rep means, calibrated frames): the float form of the mosaic
        return (4, (768, 1024), synth.phase_shifts(4), synth.gaussian_psf(), batch or 1, iters or 80,
                FLOAT_FRAMES + "C3-f4, non-integer frames: 768x1024 LR -> 3072x4096 at x4, N=16 frames, Gaussian PSF")
    raise ValueError(name)


FLOAT_FRAMES = "[float frames] "  # workload descriptions with this prefix get LR samples that are not integers (make_inputs)


def session_e2e(S, synth, n_sessions=2, reps=4, lr_hw=(768, 1024)):
    """sr_mi355x.session.process_sessions on synthetic barcode sessions written as PNG files (the reference's mono_barcodes layout,
    mono_barcodes/run_sr.py:89-130,293-351: corner{c}_rep{rr}.png, 4 corners, nominal +-0.5 px, 80 iterations per rep): decode,
    upload, Native-2x + SAA + IBP for all reps of a session in one batched call, quantise, encode, with the host work of session k + 1
    overlapped with the device work of session k.  Wall time per rep and HR-MP/s, file to file."""
    import shutil
    import tempfile
    from PIL import Image
    from sr_mi355x import session
    h, w = lr_hw
    tmp = tempfile.mkdtemp(prefix="srx_e2e_")
    try:
        rng = np.random.default_rng(3)
        base = synth.truth_image(h, w, seed=77)
        for k in range(n_sessions):
            d = os.path.join(tmp, "data", f"sheet{k}")
            os.makedirs(d)
            for r in range(reps):
                for c in range(4):
                    fr = np.clip(np.roll(base, (c + r, 2 * c + k), axis=(0, 1)) + rng.normal(0, 1, base.shape), 0, 255).astype(np.uint8)
                    Image.fromarray(fr).save(os.path.join(d, f"corner{c}_rep{r:02d}.png"))
        psf = S.make_gaussian_psf()
        sessions = session.discover_sessions(os.path.join(tmp, "data"), "mono_barcodes")
        session.process_sessions(sessions[:1], psf, os.path.join(tmp, "warm"), "mono_barcodes", verbose=False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        written = session.process_sessions(sessions, psf, os.path.join(tmp, "out"), "mono_barcodes", verbose=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = len(written)
        return {"workload": f"{n_sessions} mono_barcodes sessions x {reps} reps, {h}x{w} uint8 PNG frames -> {2 * h}x{2 * w}, 80 IBP iterations, PNG in -> 4 PNGs out per rep",
                "reps_reconstructed": n, "wall_s": round(dt, 3), "ms_per_rep": round(dt / n * 1e3, 2),
                "value": round(n * 4 * h * w / 1e6 / dt, 2), "unit": "HR-MP/s (files to files)", "path": S.last_path()}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(S, synth, lib, wl, prec, steps, warmup, seed_base, barrier=None, allmax=None, profile=True, world=1):
    """warmup + `steps` timed reconstructions (SAA + IBP) of one workload, inputs resident in HBM; then the same `steps` again,
    untimed, with HIP events around every launch of the library (recorded on its launch stream) for the iteration-level roofline
    -- a pass of its own because two event records per launch cost a path with 150 launches per step a quarter of its throughput,
    and behind one discarded step because the first profiled step after a pause measured the 12 ms kernel 1.5 ms long:
        frac = (8 + 4 N / f^2) B H W bytes [SURVEY 8d, eb = 4; 2 eb + eb N / f^2 in general]  /  kernel time per iteration  /  8 TB/s
    where the kernel time per iteration = sum over the kernels launched once per iteration of their mean duration, plus
    (duration / n_iter) of a kernel that runs all iterations in one launch (k_ibp_patch)."""
    f, lr_hw, shifts, psf, B, n_iter, desc = wl
    N, (h, w) = len(shifts), lr_hw
    H, W = h * f, w * f
    lr, _ = make_inputs(S, synth, B, f, lr_hw, shifts, psf, n_unique=min(32, B), prec=prec, seed_base=seed_base)
    if desc.startswith(FLOAT_FRAMES):  # what a rep mean looks like: fifths of a digital number
        lr = (torch.round(lr * 0.8 * 5.0) / 5.0 + 0.2).contiguous()
    torch.cuda.synchronize()

    def one_step():
        saa = S.shift_and_add_batched(lr, shifts, f, precision=prec)
        return S.ibp_batched(lr, shifts, psf, saa, f, n_iter, 0.5, precision=prec, out=saa)

    sync = barrier or torch.cuda.synchronize
    for _ in range(warmup):
        hr, errs = one_step()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        hr, errs = one_step()
    sync()
    dt = time.perf_counter() - t0
    path = S.last_path()
    if allmax is not None:
        dt = allmax(dt)
    out = {"value": world * B * H * W / 1e6 * steps / dt, "ms_per_step": dt / steps * 1e3, "path": path, "B": B, "N": N, "f": f,
           "lr_hw": [h, w], "n_iter": n_iter, "desc": desc, "lr": lr, "hr": hr, "errs": errs,
           "sane": bool(torch.isfinite(hr).all().item()) and float(errs[:, -1].mean().item()) < float(errs[:, 0].mean().item())}
    if not profile:
        return out
    lib.srx_profile_enable(1)
    one_step()
    torch.cuda.synchronize()
    lib.srx_profile_enable(1)  # drops the records of that step
    for _ in range(steps):
        one_step()
    torch.cuda.synchronize()
    eb = 4 if prec == "f32" else 8
    kernels = {}  # per STEP: launches and total time of every kernel id, averaged over the timed steps
    tot, cnt = ctypes.c_double(), ctypes.c_long()
    for kid in range(lib.srx_profile_kernel_count()):
        if lib.srx_profile_get(kid, ctypes.byref(tot), ctypes.byref(cnt)) == 0 and cnt.value:
            kernels[lib.srx_profile_kernel_name(kid).decode()] = {"launches": cnt.value // steps, "total_ms": round(tot.value / steps, 3),
                                                                  "avg_us": round(tot.value / cnt.value * 1e3, 2)}
    lib.srx_profile_enable(0)
    per_iter = {k: v["avg_us"] for k, v in kernels.items() if v["launches"] == n_iter and k != "k_ibp_patch"}
    if "k_ibp_dtile" in kernels:  # a pair of launches per iteration (byte / float form of the mosaic: an item is iterated by exactly one)
        per_iter["k_ibp_dtile"] = kernels["k_ibp_dtile"]["total_ms"] * 1e3 / n_iter
    for kn in ("k_ibp_sv", "k_ibp_sh"):  # float64 strips: the batch in chunks, n_iter + 1 vertical launches (the first and the last do half the
        if kn in kernels:                 # work) and n_iter horizontal ones per chunk
            per_iter[kn] = kernels[kn]["total_ms"] * 1e3 / n_iter
    if "k_ibp_patch" in kernels:  # all iterations of a patch in one launch
        per_iter["k_ibp_patch"] = kernels["k_ibp_patch"]["total_ms"] * 1e3 / n_iter
    out["kernels"] = kernels
    if per_iter:
        t_iter_us = sum(per_iter.values())
        it_bytes = (2 * eb + eb * N / (f * f)) * B * H * W
        dom = max(per_iter, key=per_iter.get)
        nbytes = kernel_model_bytes(dom, B, N, h, w, f, eb, n_iter)
        out["iteration"] = {"algorithmic_bytes": it_bytes, "kernels": {k: round(v, 2) for k, v in sorted(per_iter.items())},
                            "kernel_time_us": round(t_iter_us, 2), "achieved": round(it_bytes / (t_iter_us * 1e-6) / 1e9, 1),
                            "frac": round(it_bytes / (t_iter_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)}
        # k_ibp_patch runs as a pair of launches (byte / float form of the mosaic; a patch is iterated by exactly one of them, the
        # other's blocks leave at once): "one launch" of the roofline is the pair
        launch_us = (round(kernels[dom]["total_ms"] * 1e3, 2) if dom == "k_ibp_patch" else round(per_iter[dom], 2) if dom in ("k_ibp_dtile", "k_ibp_sv", "k_ibp_sh")
                     else kernels[dom]["avg_us"])
        out["dominant"] = {"kernel": dom, "avg_launch_us": launch_us, "algorithmic_bytes_per_launch": nbytes,
                           "achieved": round(nbytes / (launch_us * 1e-6) / 1e9, 1) if nbytes else None,
                           "frac": round(nbytes / (launch_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4) if nbytes else None}
    return out


def dump_outputs(d, arrays):
    """--dump-outputs: write what the timed path returned in its last step as d/<name>.npy (float32 / float64 as computed).  An array
    larger than its share of DUMP_BYTES is cut to a seeded sample of its rows (the rows of the array seen as [rows, last axis]; the
    same rows for the same shape on every run), written as d/<name>.npy [k, last axis] with the row indices in d/<name>_rows.npy."""
    os.makedirs(d, exist_ok=True)
    for name, a in arrays.items():
        if a.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"{name}: {a.dtype}")
        rows = a.reshape(-1, a.shape[-1])
        row_bytes = rows.shape[1] * rows.element_size()
        if rows.numel() * rows.element_size() <= DUMP_BYTES[name]:
            np.save(os.path.join(d, name + ".npy"), a.cpu().numpy())
            continue
        k = DUMP_BYTES[name] // (row_bytes + 8)
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rows.shape[0], k, replace=False))
        np.save(os.path.join(d, name + ".npy"), rows.index_select(0, torch.from_numpy(idx).to(rows.device)).cpu().numpy())
        np.save(os.path.join(d, name + "_rows.npy"), idx.astype(np.float64))  # exact: indices < 2^53


def kernel_source_sha16():
    """sha256 over the kernel sources this run was built from (tools/collect_traffic.py stamps its entries with the same hash)."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "enph459-super-resolution_amd", "csrc", "*"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(wname, B, prec, it):
    """HBM bytes per iteration of a workload's iteration kernels from the committed PMC passes (profiles/traffic.json, written by
    tools/collect_traffic.py from separate FETCH_SIZE / WRITE_SIZE runs of this same command line), their ratio to the algorithmic
    bytes, and where the figure comes from: profile tag, kernels, and whether the kernel sources of that profile are the ones running
    now (`stale`: the counters were collected on other code).  (None, None, None) when that workload / batch / precision was not
    profiled or a kernel of it is missing."""
    tf = os.path.join(ROOT, "profiles", "traffic.json")
    if not os.path.exists(tf):
        return None, None, None
    tj = json.load(open(tf)).get("workloads", {}).get(f"{wname}:B={B}:{prec}")
    if not tj or not all(k in tj["kernels"] for k in it["kernels"]):
        return None, None, None
    tr = sum(tj["kernels"][k]["hbm_bytes_per_iteration"] for k in it["kernels"])
    src = {"file": "profiles/traffic.json", "entry": f"{wname}:B={B}:{prec}", "profile_tag": tj.get("profile_tag"), "kernels": sorted(it["kernels"]),
           "source_sha16": tj.get("source_sha16"), "stale": tj.get("source_sha16") != kernel_source_sha16()}
    valu = {k: {q: tj["kernels"][k][q] for q in ("valu_busy", "wave_cycles_waiting")} for k in it["kernels"] if "valu_busy" in tj["kernels"][k]}
    if valu:
        src["valu"] = valu
    return (tr, round(tr / it["algorithmic_bytes"], 3), src) if tr else (None, None, None)


def cpu_baseline(synth, f, lr_hw, shifts, psf, n_iter, step):
    """The oracle (a CPU port of the reference's algorithm, float64) on a BOUNDED sample of the workload: one
    patch of at most 128x128 LR pixels, full SAA + IBP(n_iter), 1 thread like the reference (scipy.ndimage and
    pocketfft are single-threaded).  The cost is linear in pixels, so HR-MP/s of the sample is the rate."""
    from oracle import sr_oracle as O
    h, w = min(lr_hw[0], 128), min(lr_hw[1], 128)
    H, W = h * f, w * f
    truth = synth.truth_image(H, W, seed=synth.SEED_TRUTH)
    O.set_threads(1)
    lr = synth.sensor_frames(np.stack([O.forward_model(truth, psf, s, f) for s in shifts]))
    it1 = n_iter if h * w <= 64 * 64 else max(1, n_iter // 8)  # keep the sample within ~10-30 s
    t0 = time.perf_counter()
    saa = O.shift_and_add(list(lr), shifts, f)
    t_saa = time.perf_counter() - t0
    t0 = time.perf_counter()
    hr, _ = O.ibp(list(lr), shifts, psf, saa, f, it1, step)
    t_ibp = (time.perf_counter() - t0) * (n_iter / it1)
    dt = t_saa + t_ibp
    out = {"value": H * W / 1e6 / dt, "unit": "HR-MP/s", "cores": 1, "kind": "port",
           "sample": f"1 patch of the workload ({h}x{w} LR -> {H}x{W}, N={len(shifts)}, SAA + IBP: {it1} of {n_iter} "
                     f"iterations timed and scaled, float64), {dt:.1f} s-equivalent on 1 thread",
           "host_cores": os.cpu_count()}
    # all host cores (OpenMP over rows/columns inside each primitive), for scale
    nthr = min(os.cpu_count() or 1, 16)
    O.set_threads(nthr)
    it2 = max(1, it1 // 4)
    t0 = time.perf_counter()
    saa2 = O.shift_and_add(list(lr), shifts, f)
    t_saa2 = time.perf_counter() - t0
    t0 = time.perf_counter()
    O.ibp(list(lr), shifts, psf, saa2, f, it2, step)
    dt2 = t_saa2 + (time.perf_counter() - t0) * (n_iter / it2)
    O.set_threads(1)
    out["value_all_threads"] = H * W / 1e6 / dt2
    out["threads_all"] = nthr
    return out, hr, lr, it1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=0, help="items per GPU per step (default: 1024 patches for c2, 1 frame for c3_*)")
    ap.add_argument("--iters", type=int, default=0, help="IBP iterations (default: the reference's 80; 50 for c3_rgb)")
    ap.add_argument("--precision", default="f32", choices=["f32", "f64"])
    ap.add_argument("--workload", default="c2", choices=["c2", "c2_measured", "c3_mono", "c3_mono_measured", "c3_rgb", "c3_rgb_measured", "c3_f4", "c3_f4_float", "c3_f4_measured"],
                    help="c2 (default, the headline): 1024 x4 patches, N=16 phases; c3_mono / c3_rgb: the reference's own "
                         "full-frame shapes (mono_cal_target N=5 nominal f=2 3072x4096; rgb_cal_target N=4 measured f=2 1536x2048); "
                         "c3_f4: the x4 variant of SURVEY 8d, 768x1024 -> 3072x4096, all 16 phases")
    ap.add_argument("--full", action="store_true",
                    help="also the roofline (a profiled pass), the secondary legs, SAA alone, host buffers and the CPU baseline")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the profiled pass and everything after the headline but the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the secondary legs (f64 and the c3 shapes)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the last timed step's outputs (rank 0) to DIR/hr.npy and DIR/errors.npy, at most 64 MB in all "
                         "(larger arrays as a seeded sample of rows, indices in DIR/<name>_rows.npy)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    roofline_on = args.full and not args.no_roofline

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if os.environ.get("SRX_BENCH_ONE_GPU"):  # rehearsal of the N > 1 code path on a one-GPU box: all ranks on cuda:0, gloo
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    else:
        torch.cuda.set_device(0)
    if args.gpus != world and rank == 0 and world > 1:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)

    import sr_mi355x as S
    from sr_mi355x import synth, _lib

    prec = args.precision
    S.set_precision(prec)
    lib = _lib.load()
    wl = workload(synth, args.workload, args.batch, args.iters)
    f, lr_hw, shifts, psf, B, n_iter, wl_name = wl
    N, (h, w), step = len(shifts), lr_hw, 0.5
    H, W = h * f, w * f

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def allmax(dt):
        if dist is None:
            return dt
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    m = measure(S, synth, lib, wl, prec, args.steps, args.warmup, 1000 * (rank + 1), barrier, allmax,
                profile=(rank == 0 and roofline_on), world=world)
    lr, path, kernels = m["lr"], m["path"], m.get("kernels", {})
    hr_last, errs_last = m.pop("hr"), m.pop("errs")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"hr": hr_last, "errors": errs_last})
    del hr_last, errs_last

    # ---- roofline (contract field): the ITERATION-level figure of SURVEY 8d; the per-kernel view sits in dominant_kernel ----
    roofline = None
    if "iteration" in m:
        it = m["iteration"]
        roofline = {"bound": "hbm", "achieved": it["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": it["frac"],
                    "traffic": None, "traffic_ratio": None, "algorithmic_bytes_per_iteration": it["algorithmic_bytes"],
                    "kernel_time_per_iteration_us": it["kernel_time_us"], "iteration_kernels_us": it["kernels"],
                    "dominant_kernel": m.get("dominant"),
                    "note": "achieved = (8 + 4N/f^2) B per HR pixel and iteration (SURVEY 8d) x B H W / kernel time per iteration "
                            "(HIP events on the launch stream); traffic = PMC bytes of the iteration kernels per iteration"}
        roofline["traffic"], roofline["traffic_ratio"], roofline["traffic_source"] = pmc_traffic(args.workload, B, prec, it)
        if roofline["traffic"]:
            # the fraction of the HBM peak the kernel really moves (frac counts the ALGORITHMIC bytes: packed operands make it larger)
            roofline["frac_measured"] = round(roofline["traffic"] / (it["kernel_time_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
            roofline["valu"] = (roofline["traffic_source"] or {}).get("valu")

    # ---- secondary legs, timed in this same run (rank 0, N = 1): the reference's precision and its own full-frame shapes ----
    legs = None
    if rank == 0 and world == 1 and roofline_on and not args.no_secondary and args.workload == "c2":
        legs = {}
        for tag, wname, lprec, lb in (("f64", "c2", "f64", None), ("c2_measured", "c2_measured", "f32", None), ("c3_mono", "c3_mono", "f32", None), ("c3_mono_f64", "c3_mono", "f64", None),
                                      ("c3_rgb", "c3_rgb", "f32", None),
                                      ("c3_f4", "c3_f4", "f32", None), ("c3_mono_x8", "c3_mono", "f32", 8),
                                      ("c3_mono_measured", "c3_mono_measured", "f32", None), ("c3_rgb_x8", "c3_rgb", "f32", 8),
                                      ("c3_rgb_measured", "c3_rgb_measured", "f32", None), ("c3_rgb_measured_x8", "c3_rgb_measured", "f32", 8),
                                      ("c3_rgb_f64", "c3_rgb", "f64", None), ("c3_f4_x8", "c3_f4", "f32", 8),
                                      ("c3_f4_float", "c3_f4_float", "f32", None), ("c3_f4_measured", "c3_f4_measured", "f32", None)):
            lw = workload(synth, wname, lb if lb else (args.batch if wname == "c2" and args.batch else None), args.iters if wname == "c2" else None)
            r = measure(S, synth, lib, lw, lprec, 2, 1, 7000)
            legs[tag] = {"workload": r["desc"], "dtype": lprec, "batch": r["B"], "n_iter": r["n_iter"], "path": r["path"],
                         "value": round(r["value"], 2), "unit": "HR-MP/s", "ms_per_step": round(r["ms_per_step"], 3), "sane": r["sane"],
                         "iteration": r.get("iteration")}
            if r.get("iteration"):
                li = legs[tag]["iteration"]
                li["traffic"], li["traffic_ratio"], li["traffic_source"] = pmc_traffic(wname, r["B"], lprec, r["iteration"])
            del r
            torch.cuda.empty_cache()
        S.set_precision(prec)

    # ---- the real-data driver end to end: PNG files in, PNG files out (mono_barcodes layout, synthetic frames) ----
    if legs is not None:
        legs["session_e2e"] = session_e2e(S, synth)

    # ---- secondary figures: shift_and_add alone, and the same step from / to HOST buffers ----
    extras = None
    if rank == 0 and world == 1 and roofline_on:
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(3):
            S.shift_and_add_batched(lr, shifts, f, precision=prec)
        torch.cuda.synchronize()
        t_saa = (time.perf_counter() - t1) / 3
        lr_host = lr.cpu().pin_memory()
        hr_host = torch.empty((B, H, W), dtype=lr.dtype).pin_memory()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        lr_d = lr_host.cuda(non_blocking=True)
        saa_d = S.shift_and_add_batched(lr_d, shifts, f, precision=prec)
        hr_d, _ = S.ibp_batched(lr_d, shifts, psf, saa_d, f, n_iter, step, precision=prec, out=saa_d)
        hr_host.copy_(hr_d, non_blocking=True)
        torch.cuda.synchronize()
        t_host = time.perf_counter() - t1
        # the reference's own I/O types: uint8 frames in (PNG), uint8 truncated HR out (PNG): 1 byte per pixel each way.  Twice: the
        # first pass pays the first use of the cast / quantiser kernels at this size and the allocator's growth (BENCH_r02 saw 92.7 ms
        # where a warm pass takes 17), the second is the steady state; both are reported
        lr_u8 = lr.to(torch.uint8).cpu().pin_memory()
        hr_u8 = torch.empty((B, H, W), dtype=torch.uint8).pin_memory()
        t_u8s = []
        for _ in range(2):
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lr_d = S.u8_to_float(lr_u8.cuda(non_blocking=True), precision=prec)
            saa_d = S.shift_and_add_batched(lr_d, shifts, f, precision=prec)
            hr_d, _ = S.ibp_batched(lr_d, shifts, psf, saa_d, f, n_iter, step, precision=prec, out=saa_d)
            hr_u8.copy_(S.quantize_u8(hr_d), non_blocking=True)
            torch.cuda.synchronize()
            t_u8s.append(time.perf_counter() - t1)
        t_u8 = t_u8s[1]
        del lr_u8, hr_u8
        extras = {"saa_only_hr_mp_per_s": round(B * H * W / 1e6 / t_saa, 1), "saa_only_ms": round(t_saa * 1e3, 3),
                  "host_u8_hr_mp_per_s": round(B * H * W / 1e6 / t_u8, 1), "host_u8_ms": round(t_u8 * 1e3, 3),
                  "host_u8_first_pass_ms": round(t_u8s[0] * 1e3, 3),
                  "host_u8_note": "pinned uint8 LR in, device cast, step, truncating uint8 quantiser, pinned uint8 HR out",
                  "host_buffers_hr_mp_per_s": round(B * H * W / 1e6 / t_host, 1), "host_buffers_ms": round(t_host * 1e3, 3),
                  "host_buffers_note": "pinned host LR in, pinned host HR out, H2D + step + D2H on one stream; never the headline value"}
        del lr_host, hr_host, lr_d, saa_d, hr_d
    if extras is not None and legs is not None:
        extras.update(legs)
    elif legs is not None:
        extras = legs

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu, hr_cpu, lr_cpu, it_cpu = cpu_baseline(synth, f, lr_hw, shifts, psf, n_iter, step)
        # parity spot check of the same patch on the GPU (the oracle is only the checker here)
        saa_g = S.shift_and_add_batched(torch.from_numpy(lr_cpu)[None], shifts, f, precision=prec)
        hr_g, _ = S.ibp_batched(torch.from_numpy(lr_cpu)[None], shifts, psf, saa_g, f, it_cpu, step, precision=prec)
        cpu["psnr_gpu_vs_cpu_db"] = round(synth.psnr(hr_g[0].double().cpu().numpy(), hr_cpu), 2)

    if rank == 0:
        line = {
            "metric": f"HR megapixels/sec at x{f} upscale (SAA + {n_iter}-iteration IBP reconstruction)",
            "value": round(m["value"], 2), "unit": "HR-MP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(m["ms_per_step"], 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": prec, "data": "synthetic",
            "config": {"workload": wl_name,
                       "patches_per_gpu": B, "global_patches": world * B, "factor": f, "frames": N, "lr_patch": [h, w],
                       "n_iter": n_iter, "path": path, "parallelism": f"patch-sharded x{world}, no collective"},
            "hr_mp_iter_per_s": round(m["value"] * n_iter, 1), "sane": m["sane"],
            "roofline": roofline, "kernels": kernels, "secondary": extras, "cpu_baseline": cpu,
        }
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
