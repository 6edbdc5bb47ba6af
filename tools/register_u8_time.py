#!/usr/bin/env python3
"""HIP-event time per registration of uint8 frames, three ways:

  (a) what a session did before srx_register_u8: srx_u8_to_f64 (the loaders' float64), the cast to the compute precision (a torch copy;
      none in f64), srx_register_T
  (b) srx_u8_to_T into a buffer the caller owns, then srx_register_T
  (c) srx_register_u8_T on the bytes

on [1, 5, 1536, 2048] (a mono_cal_target session) and [8, 4, 768, 1024] (the reps of a barcode session, red planes), in f32 and f64, search 2,
border 8, with 10 iterations at tol 1e-4 (as used) and with n_iter = 0 (prefilter + coarse search + score pass: the fixed part).  Frames are
tools/register_time.py's smooth scene shifted by the jittered nominal table and rounded to uint8.  One event pair per call, the median of
--iters calls after --warmup; (a), (b), (c) alternate in one process and the whole round is repeated --rounds times: the spread of a
variant is max - min of its medians over the rounds.  (b) and (c) are compared bit for bit first.

Also reported, counted from shapes: the bytes each form's conversion moves, the bytes the registration passes read from the frames, and
the peak device memory of frames + converted copies + workspace.

--label NAME is stored in the JSON (the coarse-kernel ablation ran this tool through SRX_LIB on a library built with -DSRX_REG_COARSE_PLAIN,
a switch that was removed once the verdict was in: the commit before its removal builds it).
--profile-run runs 20 calls of (b) and 20 of (c) on the mono_cal_target shape in f32 and exits: the workload for
`rocprofv3 --kernel-trace --stats -- python tools/register_u8_time.py --profile-run` (nothing else traced).

Exits non-zero where (c) is slower than (b) by more than the spread of (b).

usage: tools/register_u8_time.py [--iters N] [--warmup N] [--rounds N] [--json PATH] [--label NAME] [--profile-run]
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

SEARCH, BORDER, N_ITER, TOL = 2, 8, 10, 1e-4
SHAPES = {"mono_cal_target": (1, 1536, 2048, synth.NOMINAL_5), "barcode_reps": (8, 768, 1024, synth.NOMINAL_4)}
NPAD = 12


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


def scene(H, W):
    """tools/register_time.py's scene: uniform noise under two 9 x 9 box filters, stretched to [0, 255]"""
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand((1, 1, H + 64, W + 64), generator=g, device="cuda", dtype=torch.float64)
    k = torch.ones((1, 1, 9, 9), device="cuda", dtype=torch.float64) / 81.0
    x = torch.nn.functional.conv2d(torch.nn.functional.conv2d(x, k), k)[0, 0]
    x = (x - x.min()) / (x.max() - x.min()) * 255.0
    return x[:H, :W].contiguous()


def frames_u8(B, H, W, table):
    base = scene(H, W)
    rng = np.random.default_rng(5)
    items = []
    for _ in range(B):
        jit = rng.uniform(-0.1, 0.1, np.shape(table))
        jit[0] = 0.0
        items.append(torch.stack([api.shift_batched(base[None], s, precision="f64")[0] for s in np.asarray(table) + jit]))
    return torch.stack(items).round().clamp(0, 255).to(torch.uint8).contiguous()


class Case:
    def __init__(self, lib, name, prec):
        B, H, W, table = SHAPES[name]
        self.lib, self.name, self.prec, self.B, self.N, self.H, self.W = lib, name, prec, B, len(table), H, W
        self.x8 = frames_u8(B, H, W, table)
        self.n = self.x8.numel()
        self.dt, self.eb = api._TORCH_DT[prec], api._ELEM[prec]
        self.x64 = torch.empty(self.x8.shape, dtype=torch.float64, device="cuda")  # (a)'s loader copy
        self.xT = torch.empty(self.x8.shape, dtype=self.dt, device="cuda")         # (b)'s converted copy
        self.ws_n = lib.srx_register_workspace_bytes(self.eb, B, self.N, H, W, SEARCH)
        self.ws = torch.empty(self.ws_n, dtype=torch.uint8, device="cuda")
        self.init = np.ascontiguousarray(table, dtype=np.float64)
        self.out = {v: (torch.empty((B, self.N, 2), dtype=torch.float64, device="cuda"), torch.empty((B, self.N), dtype=torch.float64, device="cuda"),
                        torch.empty((B, self.N), dtype=torch.int32, device="cuda")) for v in "abc"}
        self.st = api._stream()

    def _register(self, name, x, v, n_iter):
        sh, sc, st = self.out[v]
        _lib.check(getattr(self.lib, f"{name}_{self.prec}")(api._p(x), self.B, self.N, self.H, self.W, 0, self.init.ctypes.data_as(_lib._HD), SEARCH, BORDER,
                                                           n_iter, TOL, api._p(sh), api._p(sc), api._p(st), api._p(self.ws), ctypes.c_size_t(self.ws_n),
                                                           self.st), name)

    def run(self, v, n_iter):
        if v == "a":
            _lib.check(self.lib.srx_u8_to_f64(api._p(self.x8), ctypes.c_size_t(self.n), api._p(self.x64), self.st), "srx_u8_to")
            self._register("srx_register", self.x64.to(self.dt), v, n_iter)
        elif v == "b":
            _lib.check(getattr(self.lib, f"srx_u8_to_{self.prec}")(api._p(self.x8), ctypes.c_size_t(self.n), api._p(self.xT), self.st), "srx_u8_to")
            self._register("srx_register", self.xT, v, n_iter)
        else:
            self._register("srx_register_u8", self.x8, v, n_iter)

    def counted(self, n_iter_run):
        """bytes from shapes: conversion traffic, frame bytes the registration passes read, peak device memory"""
        n, eb, nf = self.n, self.eb, self.B * (self.N - 1)
        m = BORDER + SEARCH + 2
        crop = (self.H - 2 * m) * (self.W - 2 * m)
        # samples read from the frames: k_reg_pad (every moving frame once, with its 12-sample edge pad), the coarse chunks and their windows
        # (reference crop + moving crop, halo not counted), one reference crop per Gauss-Newton pass and one for the score pass
        reads = nf * (self.H + 2 * NPAD) * (self.W + 2 * NPAD) + nf * 2 * crop + nf * (n_iter_run + 1) * crop
        conv = {"a": n + 8 * n + (8 * n + eb * n if eb != 8 else 0), "b": n + eb * n, "c": 0}
        copies = {"a": 8 * n + (eb * n if eb != 8 else 0), "b": eb * n, "c": 0}
        return dict(conversion_bytes=conv, frame_read_bytes={"a": reads * eb, "b": reads * eb, "c": reads},
                    peak_device_bytes={v: n + copies[v] + self.ws_n for v in "abc"}, workspace_bytes=self.ws_n)


def profile_run(lib):
    c = Case(lib, "mono_cal_target", "f32")
    for v in "bc":
        for _ in range(20):
            c.run(v, N_ITER)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--label", default="shipped")
    ap.add_argument("--profile-run", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("register_u8_time.py needs a GPU")
    lib = _lib.load()
    if a.profile_run:
        return profile_run(lib)
    rows, bad = [], []
    for name in SHAPES:
        for prec in ("f32", "f64"):
            c = Case(lib, name, prec)
            for n_iter in (N_ITER, 0):
                for v in "abc":
                    c.run(v, n_iter)
                torch.cuda.synchronize()
                for v in "bc":  # the same bits, whatever the way in
                    assert all(torch.equal(p, q) for p, q in zip(c.out[v], c.out["a"])), (name, prec, n_iter, v)
                med = {v: [] for v in "abc"}
                for _ in range(max(a.rounds, 3)):
                    for v in "abc":
                        med[v].append(median_us(lambda: c.run(v, n_iter), a.iters, a.warmup))
                best = {v: min(m) for v, m in med.items()}
                spread = {v: max(m) - min(m) for v, m in med.items()}
                rows.append(dict(shape=name, B=c.B, N=c.N, H=c.H, W=c.W, precision=prec, n_iter=n_iter, us_medians=med, us_best=best, us_spread=spread,
                                 c_over_b=best["c"] / best["b"], c_over_a=best["c"] / best["a"], status=c.out["c"][2].cpu().numpy().tolist(),
                                 **c.counted(n_iter)))
                print(f"{name:>16} {prec} n_iter={n_iter:<2} " + "  ".join(f"({v}) {best[v]:8.1f} us +{spread[v]:5.1f}" for v in "abc") +
                      f"   c/b {best['c'] / best['b']:.3f}  c/a {best['c'] / best['a']:.3f}")
                if best["c"] > best["b"] + spread["b"]:
                    bad.append(f"{name} {prec} n_iter={n_iter}: (c) {best['c']:.1f} us > (b) {best['b']:.1f} us + spread {spread['b']:.1f} us")
            del c
            torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fp:
            json.dump(dict(device=torch.cuda.get_device_name(0), label=a.label, iters=a.iters, warmup=a.warmup, rounds=max(a.rounds, 3), search=SEARCH,
                           border=BORDER, tol=TOL, rows=rows, failed=bad), fp, indent=1)
    if bad:
        raise SystemExit("register_u8_time: " + "; ".join(bad))


if __name__ == "__main__":
    main()
