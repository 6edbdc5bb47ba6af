#!/usr/bin/env python3
"""What the device PNG coder (api.png_deflate / srx_png_deflate_*) costs beside the host writer (session.write_png_u8):

  * device time of srx_png_deflate_f32 on [3, 3072, 4096] and [3, 1536, 2048] float planes (a reconstruction's three HR outputs): HIP
    events around the call, the best and the median of --iters calls after --warmup, --rounds rounds; the spread is that of the rounds' bests;
  * write_png_u8 on the same three quantised planes, one thread, host clock, best of --host-iters;
  * the stream sizes beside the host writer's zlib streams;
  * bench.py's session_e2e workload (2 mono_barcodes sessions x 4 reps of 768 x 1024 frames, files to files) through
    session.process_sessions with device_png off and on, alternating in one process, --e2e-rounds rounds.

The planes are synth.truth_image plus N(0, 1) noise: the statistics of a reconstruction, not its values.

usage: tools/png_time.py [--iters N] [--warmup N] [--rounds N] [--host-iters N] [--e2e-rounds N] [--no-e2e] [--json PATH]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "enph459-super-resolution_amd"))
import sr_mi355x as S  # noqa: E402
from sr_mi355x import api, session, synth  # noqa: E402

SHAPES = ((3, 3072, 4096), (3, 1536, 2048))


def planes(B, H, W):
    rng = np.random.default_rng(5)
    base = synth.truth_image(H, W, seed=9)
    return np.stack([np.roll(base, (7 * b, 3 * b), axis=(0, 1)) + rng.normal(0.0, 1.0, (H, W)) for b in range(B)])


def event_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    t = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return float(min(t)), float(np.median(t))


def host_stream_bytes(a):
    raw = np.empty((a.shape[0], a.shape[1] + 1), np.uint8)
    raw[:, 0] = 2
    raw[0, 1:] = a[0]
    np.subtract(a[1:], a[:-1], out=raw[1:, 1:])
    c = zlib.compressobj(session.PNG_COMPRESS_LEVEL, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return len(c.compress(raw) + c.flush())


def encode_rows(a):
    rows = []
    for B, H, W in SHAPES:
        x64 = planes(B, H, W)
        x = torch.from_numpy(x64).to("cuda", torch.float32)
        lib = api._lib.load()
        streams = torch.empty((B, lib.srx_png_stream_bound(H, W)), dtype=torch.uint8, device="cuda")
        lengths = torch.empty((B,), dtype=torch.int64, device="cuda")
        ws, wsp, wsn = api._ws(lib.srx_png_scratch_bytes(B, H, W))
        call = lambda: api._lib.check(lib.srx_png_deflate_f32(api._p(x), B, H, W, api._p(streams), api._p(lengths), wsp, wsn, api._stream()), "png")  # noqa: E731
        best, med = zip(*[event_us(call, a.iters, a.warmup) for _ in range(a.rounds)])
        q = api.quantize_u8(x).cpu().numpy()
        n = lengths.cpu().tolist()
        host = streams.cpu().numpy()
        for b in range(B):  # what is timed is also right
            raw = zlib.decompress(host[b, :n[b]].tobytes())
            assert np.array_equal(np.cumsum(np.frombuffer(raw, np.uint8).reshape(H, W + 1)[:, 1:], axis=0, dtype=np.uint8), q[b])
        with tempfile.TemporaryDirectory() as d:
            t_host = []
            for _ in range(a.host_iters):
                t0 = time.perf_counter()
                for b in range(B):
                    session.write_png_u8(os.path.join(d, f"{b}.png"), q[b])
                t_host.append((time.perf_counter() - t0) * 1e3)
        host_bytes = [host_stream_bytes(q[b]) for b in range(B)]
        rows.append(dict(B=B, H=H, W=W, raw_bytes=B * H * (W + 1), us_device_best=float(min(best)), us_device_best_rounds=list(best),
                         us_device_median_rounds=list(med), spread_best=(max(best) - min(best)) / min(best),
                         ms_write_png_u8_one_thread_best=float(min(t_host)), ms_write_png_u8_rounds=t_host,
                         host_ms_over_device_ms=float(min(t_host)) / (float(min(best)) * 1e-3),
                         stream_bytes_device=n, stream_bytes_host=host_bytes, device_over_host_bytes=float(sum(n)) / float(sum(host_bytes)),
                         scratch_bytes=int(wsn.value)))
        del x, streams, ws
        torch.cuda.empty_cache()
    return rows


def e2e_leg(rounds, n_sessions=2, reps=4, lr_hw=(768, 1024)):
    """bench.py's session_e2e workload (same frames, same calls), once per round with device_png off and on"""
    from PIL import Image
    h, w = lr_hw
    tmp = tempfile.mkdtemp(prefix="srx_png_e2e_")
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
        t = {False: [], True: []}
        for flag in (False, True):
            session.process_sessions(sessions[:1], psf, os.path.join(tmp, f"warm{int(flag)}"), "mono_barcodes", verbose=False, device_png=flag)
        for rnd in range(rounds):
            for flag in (False, True):
                out = os.path.join(tmp, f"out{rnd}_{int(flag)}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = session.process_sessions(sessions, psf, out, "mono_barcodes", verbose=False, device_png=flag)
                torch.cuda.synchronize()
                t[flag].append((time.perf_counter() - t0) / len(written) * 1e3)
                shutil.rmtree(out, ignore_errors=True)
        return dict(workload=f"{n_sessions} mono_barcodes sessions x {reps} reps, {h}x{w} frames, 80 IBP iterations, files to files",
                    host_threads=session._host_threads(), rounds=rounds, ms_per_rep_host_png_rounds=t[False], ms_per_rep_device_png_rounds=t[True],
                    ms_per_rep_host_png=float(np.median(t[False])), ms_per_rep_device_png=float(np.median(t[True])),
                    host_over_device=float(np.median(t[False]) / np.median(t[True])),
                    faster_beyond_spread=bool(max(t[True]) < min(t[False])))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_time.py needs a GPU")
    rows = encode_rows(a)
    for r in rows:
        print(f"[{r['B']}, {r['H']}, {r['W']}] float32: device {r['us_device_best']:.0f} us (best; spread of the rounds {100 * r['spread_best']:.1f} %), "
              f"write_png_u8 on one thread {r['ms_write_png_u8_one_thread_best']:.1f} ms = {r['host_ms_over_device_ms']:.0f} x; "
              f"streams {r['device_over_host_bytes']:.4f} x the host writer's bytes")
    e2e = None if a.no_e2e else e2e_leg(a.e2e_rounds)
    if e2e:
        print(f"session_e2e: {e2e['ms_per_rep_host_png']:.2f} ms per rep with the host writer, {e2e['ms_per_rep_device_png']:.2f} ms with device_png "
              f"({e2e['host_over_device']:.2f} x{'' if e2e['faster_beyond_spread'] else ', NOT beyond the spread'}), {e2e['host_threads']} host threads")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rounds=a.rounds, rows=rows, session_e2e=e2e), f, indent=1)


if __name__ == "__main__":
    main()
