#!/usr/bin/env python3
"""HIP-event time per call of srx_ibp_items_f32 against the shared-table call it stands in for: float32, x2, N = 4, 768 x 1024 LR frames
(rgb_cal_target's shape), 50 iterations, Gaussian PSF, B = 8, eight tables = synth.MEASURED_4 plus a seeded jitter of +-0.05 px.

  (a) eight B = 1 calls of srx_ibp_f32, one per table        (what a caller with registered frames had to do)
  (b) one srx_ibp_items_f32 call on the eight tables
  (c) one srx_ibp_f32 call of B = 8 on the first table       (the figure (b) should reach)
  (d) = (c) with another build of the library (--ref-lib: the parent commit's libsrx.so), the same box

Every measurement is a process of its own under its own time limit (`timeout`): a round measures (c), (a), (b) in one process and (d) in
another, (c) first in its process as (d) is in its own, and the rounds interleave the two builds.  3 warm-up calls, 20 timed calls per figure; min - max over the rounds are reported.
The first step that fails ends the run with its status.

usage: tools/items_time.py [--rounds 5] [--iters 20] [--warmup 3] [--ref-lib PATH] [--json PATH]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "enph459-super-resolution_amd")
H_LR, W_LR, N, B, F, N_ITER, STEP = 768, 1024, 4, 8, 2, 50, 0.5
STEP_TIMEOUT = 240  # seconds per measuring process


def tables():
    import numpy as np
    sys.path.insert(0, PKG)
    from sr_mi355x import synth
    base = np.asarray(synth.MEASURED_4, dtype=np.float64)
    return np.ascontiguousarray(base[None] + np.random.default_rng(8).uniform(-0.05, 0.05, (B, N, 2)))


def measure(lib_path, legs, iters, warmup):
    """one process: the legs named in `legs` on the library at lib_path (bound here, symbol by symbol: a reference build has no items call)"""
    import numpy as np
    import torch  # before the library: it must bind to torch's HIP runtime
    sys.path.insert(0, PKG)
    from sr_mi355x import synth
    lib = ctypes.CDLL(lib_path)
    I, P, D, Z, U, HD = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_size_t, ctypes.c_uint, ctypes.POINTER(ctypes.c_double)
    ibp_args = [P, I, I, I, I, HD, HD, I, I, P, I, I, I, I, D, P, P, P, Z, P, U]
    ws_args = [I, I, I, I, I, I, I, I, HD, HD, I, I, U]
    lib.srx_ibp_f32.restype, lib.srx_ibp_f32.argtypes = I, ibp_args
    lib.srx_ibp_workspace_bytes_for.restype, lib.srx_ibp_workspace_bytes_for.argtypes = Z, ws_args
    if "b" in legs:
        lib.srx_ibp_items_f32.restype, lib.srx_ibp_items_f32.argtypes = I, ibp_args
        lib.srx_ibp_items_workspace_bytes_for.restype, lib.srx_ibp_items_workspace_bytes_for.argtypes = Z, ws_args
    lib.srx_last_path.restype = ctypes.c_char_p
    H, W = H_LR * F, W_LR * F
    g = torch.Generator(device="cuda").manual_seed(3)
    scene = torch.rand((B, 1, H_LR + 16, W_LR + 16), generator=g, device="cuda")
    k9 = torch.ones((1, 1, 9, 9), device="cuda") / 81.0
    scene = torch.nn.functional.conv2d(torch.nn.functional.conv2d(scene, k9), k9)
    scene = (scene - scene.min()) / (scene.max() - scene.min()) * 255.0
    lr = (scene + 2.0 * torch.randn((B, N, H_LR, W_LR), generator=g, device="cuda")).clamp(0, 255).contiguous()
    hr0 = lr.mean(1).repeat_interleave(F, 1).repeat_interleave(F, 2).contiguous()
    hr = torch.empty_like(hr0)
    errs = torch.empty((B, N_ITER), dtype=torch.float64, device="cuda")
    tabs = tables()
    psf = np.ascontiguousarray(synth.gaussian_psf(), dtype=np.float64)
    kp, kh, kw = psf.ctypes.data_as(HD), psf.shape[0], psf.shape[1]
    tp = lambda b: tabs[b].ctypes.data_as(HD)  # noqa: E731
    need = max(lib.srx_ibp_workspace_bytes_for(4, B, N, H_LR, W_LR, H, W, F, tp(0), kp, kh, kw, 0),
               lib.srx_ibp_items_workspace_bytes_for(4, B, N, H_LR, W_LR, H, W, F, tabs.ctypes.data_as(HD), kp, kh, kw, 0) if "b" in legs else 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    fr, pl = N * H_LR * W_LR * 4, H * W * 4

    def shared(b0, nb, table):
        return lib.srx_ibp_f32(ctypes.c_void_p(lr.data_ptr() + b0 * fr), nb, N, H_LR, W_LR, table, kp, kh, kw, ctypes.c_void_p(hr0.data_ptr() + b0 * pl),
                               H, W, F, N_ITER, STEP, ctypes.c_void_p(hr.data_ptr() + b0 * pl), ctypes.c_void_p(errs.data_ptr() + b0 * N_ITER * 8),
                               p(ws), need, None, 0)

    def leg_a():
        for b in range(B):
            st = shared(b, 1, tp(b))
            if st:
                return st
        return 0

    calls = {"a": leg_a, "b": lambda: lib.srx_ibp_items_f32(p(lr), B, N, H_LR, W_LR, tabs.ctypes.data_as(HD), kp, kh, kw, p(hr0), H, W, F, N_ITER, STEP,
                                                            p(hr), p(errs), p(ws), need, None, 0),
             "c": lambda: shared(0, B, tp(0))}
    out = {}
    for leg in legs:
        fn = calls[leg]
        for _ in range(warmup):
            assert fn() == 0, f"leg {leg}: status"
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            assert fn() == 0, f"leg {leg}: status"
        e1.record()
        torch.cuda.synchronize()
        out[leg] = dict(ms=e0.elapsed_time(e1) / iters, path=lib.srx_last_path().decode(), mse_last=float(errs[:, -1].mean()))
    out["device"] = torch.cuda.get_device_name(0)
    print("ITEMS_TIME " + json.dumps(out))


def child(lib_path, legs, a):
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), "--measure", legs, "--lib", lib_path, "--iters", str(a.iters),
           "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print(r.stdout[-2000:])
        raise SystemExit(r.returncode)  # nothing more is started after a step that failed
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("ITEMS_TIME ")][-1]
    return json.loads(line[len("ITEMS_TIME "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-lib", default=None, help="another build of libsrx.so for leg (d), e.g. the parent commit's")
    ap.add_argument("--json", default=None)
    ap.add_argument("--measure", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=os.path.join(PKG, "sr_mi355x", "libsrx.so"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.measure:
        return measure(a.lib, a.measure, a.iters, a.warmup)
    runs = {"a": [], "b": [], "c": [], "d": []}
    paths, device = {}, None
    for r in range(a.rounds):
        got = child(a.lib, "cab", a)  # (c) first, as in (d)'s process: both measured on a device in the same state
        device = got["device"]
        for leg in "abc":
            runs[leg].append(got[leg]["ms"])
            paths[leg] = got[leg]["path"]
        if a.ref_lib:
            d = child(os.path.abspath(a.ref_lib), "c", a)["c"]
            runs["d"].append(d["ms"])
            paths["d"] = d["path"]
        print(f"round {r}: " + "  ".join(f"({leg}) {runs[leg][-1]:8.3f} ms" for leg in "abcd" if runs[leg]), flush=True)
    rows = {leg: dict(ms_runs=v, ms_min=min(v), ms_max=max(v), path=paths[leg]) for leg, v in runs.items() if v}
    what = {"a": "8 x srx_ibp_f32, B = 1, one per table", "b": "srx_ibp_items_f32, B = 8, eight tables", "c": "srx_ibp_f32, B = 8, the first table",
            "d": "(c) with --ref-lib"}
    for leg, x in rows.items():
        print(f"({leg}) {what[leg]:42s} {x['ms_min']:8.3f} - {x['ms_max']:8.3f} ms per call  [{x['path']}]")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=device, shape=dict(B=B, N=N, h=H_LR, w=W_LR, factor=F, n_iter=N_ITER, precision="f32"),
                           calls=dict(warmup=a.warmup, timed=a.iters, rounds=a.rounds), legs={leg: dict(what=what[leg], **x) for leg, x in rows.items()}),
                      f, indent=1)


if __name__ == "__main__":
    main()
