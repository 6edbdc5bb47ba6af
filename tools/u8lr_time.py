#!/usr/bin/env python3
"""HIP-event time per call of shift_and_add and ibp (float32 state) on uint8 frames, three ways:

  (a) srx_saa_f32 / srx_ibp_f32 on float32 frames                                   -- the caller converted long ago
  (b) srx_u8_to_f32 into a buffer the caller owns, then (a)                         -- what a caller holding bytes had to do
  (c) srx_saa_u8lr_f32 / srx_ibp_u8lr_f32 on the bytes                              -- this entry point
  (c bytes) ibp on the patch path: the same with SRX_FLAG_DIAG_U8_BYTE_LOADS (k_patch_build's other read shape, one byte per lane)

on the C2 patch batch (B = 1024, N = 16, 64 x 64, x4, Gaussian PSF), the mono frame (B = 1, N = 5, 1536 x 2048, x2) and a barcode batch
(B = 8, N = 4, 1536 x 2048, x2); ibp at n_iter = 1 and 80.  One event pair per call, the median of --iters calls after --warmup; the
variants alternate in one process and (a) is timed twice per round, so the spread of its repeated medians is at hand.  The kernels that
read the frames are timed one by one through srx_profile_get in a call of their own.  Every variant's result is compared bit for bit.

Also reported, computed from shapes: the bytes each variant's passes over the frames move, and the device memory the frames hold; and for
C2 the host-to-device time of the frames from pinned memory as float32 and as uint8.

Prints one line per workload and call; --json PATH writes everything.  Exits non-zero where (c) is slower than (a) by more than the
spread of (a)'s own medians, or not faster than (b).

usage: tools/u8lr_time.py [--iters N] [--warmup N] [--json PATH] [--only c2|mono|barcodes]
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

WORKLOADS = {
    # name: (B, N, (h, w), factor, shifts)
    "c2": (1024, 16, (64, 64), 4, synth.phase_shifts(4)),
    "mono": (1, 5, (1536, 2048), 2, synth.NOMINAL_5),
    "barcodes": (8, 4, (1536, 2048), 2, synth.NOMINAL_4),
}
LR_KERNELS = ("k_mosaic_build", "k_prefilter_small", "k_prefilter_tile", "k_prefilter_axis0", "k_prefilter_axis1", "k_patch_build", "k_patch_build_float")


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


def kernel_times(lib, fn):
    """one profiled call -> {kernel name: (us, launches)} of the kernels that ran"""
    lib.srx_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    out = {}
    for i in range(lib.srx_profile_kernel_count()):
        ms, n = ctypes.c_double(), ctypes.c_long()
        _lib.check(lib.srx_profile_get(i, ctypes.byref(ms), ctypes.byref(n)), "srx_profile_get")
        if n.value:
            out[lib.srx_profile_kernel_name(i).decode()] = (ms.value * 1e3, n.value)
    lib.srx_profile_enable(0)
    return out


def h2d_us(host, dev, iters, warmup):
    return median_us(lambda: dev.copy_(host, non_blocking=True), iters, warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("u8lr_time.py needs a GPU")
    lib, st = _lib.load(), api._stream()
    psf = synth.gaussian_psf()
    k, kp = api._host_f64(psf)
    rows, bad = [], []
    for name, (B, N, (h, w), f, shifts) in WORKLOADS.items():
        if a.only and a.only != name:
            continue
        H, W = h * f, w * f
        sh, shp = api._host_f64(shifts, (N, 2))
        g = torch.Generator(device="cuda").manual_seed(459)
        lr8 = torch.randint(0, 256, (B, N, h, w), generator=g, device="cuda", dtype=torch.uint8)
        lrf = lr8.float()
        stage = torch.empty_like(lrf)  # (b)'s converted copy
        n = lr8.numel()
        out = {v: torch.empty((B, H, W), dtype=torch.float32, device="cuda") for v in ("a", "b", "c", "c_bytes")}
        errs = {v: torch.empty((B, 80), dtype=torch.float64, device="cuda") for v in out}
        ws_n = max(lib.srx_saa_u8lr_workspace_bytes(4, B, N, h, w, f), lib.srx_ibp_u8lr_workspace_bytes_for(4, B, N, h, w, H, W, f, shp, kp, 7, 7, 0))
        ws = torch.empty(ws_n, dtype=torch.uint8, device="cuda")
        wp, wn = api._p(ws), ctypes.c_size_t(ws_n)
        path = lib.srx_ibp_path_for(4, N, h, w, H, W, f, shp, kp, 7, 7, 0).decode()

        def saa(v):
            if v == "b":
                _lib.check(lib.srx_u8_to_f32(api._p(lr8), ctypes.c_size_t(n), api._p(stage), st), "srx_u8_to")
            if v in ("a", "b"):
                _lib.check(lib.srx_saa_f32(api._p(lrf if v == "a" else stage), B, N, h, w, shp, f, api._p(out[v]), wp, wn, st, 0), "srx_saa")
            else:
                _lib.check(lib.srx_saa_u8lr_f32(api._p(lr8), B, N, h, w, shp, f, api._p(out[v]), wp, wn, st, 0), "srx_saa_u8lr")

        saa("a")
        init = out["a"].clone()

        def ibp(v, n_iter):
            if v == "b":
                _lib.check(lib.srx_u8_to_f32(api._p(lr8), ctypes.c_size_t(n), api._p(stage), st), "srx_u8_to")
            if v in ("a", "b"):
                _lib.check(lib.srx_ibp_f32(api._p(lrf if v == "a" else stage), B, N, h, w, shp, kp, 7, 7, api._p(init), H, W, f, n_iter, 0.5, api._p(out[v]),
                                           api._p(errs[v]), wp, wn, st, 0), "srx_ibp")
            else:
                _lib.check(lib.srx_ibp_u8lr_f32(api._p(lr8), B, N, h, w, shp, kp, 7, 7, api._p(init), H, W, f, n_iter, 0.5, api._p(out[v]), api._p(errs[v]),
                                                wp, wn, st, _lib.FLAG_DIAG_U8_BYTE_LOADS if v == "c_bytes" else 0), "srx_ibp_u8lr")

        shapes = ("a", "b", "c") + (("c_bytes",) if path == "patch" else ())  # (k_patch_build has two read shapes)
        calls = [("saa", saa, ("a", "b", "c"))] + [(f"ibp n_iter={it}", (lambda v, it=it: ibp(v, it)), shapes) for it in (1, 80)]
        for cname, fn, variants in calls:
            for v in variants:  # the same bits, whatever the way in
                fn(v)
            torch.cuda.synchronize()
            for v in variants[1:]:
                assert torch.equal(out[v], out["a"]), (name, cname, v)
                if cname != "saa":
                    it = int(cname.split("=")[1])
                    assert torch.equal(errs[v][:, :it], errs["a"][:, :it]), (name, cname, v)
            med = {v: [] for v in variants}
            for _ in range(2):  # two rounds, the variants alternating; (a) twice per round
                for v in ("a",) + variants:
                    med[v].append(median_us(lambda: fn(v), a.iters, a.warmup))
            best = {v: min(m) for v, m in med.items()}
            spread = max(med["a"]) - min(med["a"])
            kern = {v: {kn: t for kn, t in kernel_times(lib, lambda: fn(v)).items() if kn in LR_KERNELS} for v in variants}
            eb = 4
            passes = {"a": n * eb, "b": n * (1 + eb) + n * eb, "c": n, "c_bytes": n}  # one pass over the frames (+ the conversion's read and write)
            rows.append(dict(workload=name, call=cname, path="mosaic" if cname == "saa" else path, B=B, N=N, h=h, w=w, factor=f,
                             us_medians=med, us_best=best, spread_of_a_us=spread, lr_kernels_us=kern,
                             lr_pass_bytes={v: passes[v] for v in variants},
                             frame_memory_bytes={"a": n * eb, "b": n + n * eb, "c": n}))
            line = "  ".join(f"({v}) {best[v]:9.1f} us" for v in variants)
            print(f"{name:>8} {cname:<14} {line}   spread of (a) {spread:6.1f} us   c/a {best['c'] / best['a']:.3f}  c/b {best['c'] / best['b']:.3f}")
            for v in variants:
                print(f"{'':>8} {'':<14} ({v}) frame kernels: " + ", ".join(f"{kn} {t:.1f} us x{cnt}" for kn, (t, cnt) in kern[v].items()))
            if best["c"] > best["a"] + spread:
                bad.append(f"{name} {cname}: (c) {best['c']:.1f} us > (a) {best['a']:.1f} us + spread {spread:.1f} us")
            if best["c"] >= best["b"]:
                bad.append(f"{name} {cname}: (c) {best['c']:.1f} us is not faster than (b) {best['b']:.1f} us")
        if name == "c2":
            hf, h8 = torch.empty(lrf.shape, dtype=torch.float32, pin_memory=True), torch.empty(lr8.shape, dtype=torch.uint8, pin_memory=True)
            hf.copy_(lrf), h8.copy_(lr8)
            tf, t8 = h2d_us(hf, lrf, a.iters, a.warmup), h2d_us(h8, lr8, a.iters, a.warmup)
            rows.append(dict(workload=name, call="host to device, pinned", us_float32=tf, us_uint8=t8, bytes_float32=n * 4, bytes_uint8=n))
            print(f"{name:>8} upload from pinned memory: float32 {tf:9.1f} us ({n * 4 / 1e6:.0f} MB), uint8 {t8:9.1f} us ({n / 1e6:.0f} MB)")
        del lr8, lrf, stage, out, errs, ws, init
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rows=rows, failed=bad), fp, indent=1)
    if bad:
        raise SystemExit("u8lr_time: " + "; ".join(bad))


if __name__ == "__main__":
    main()
