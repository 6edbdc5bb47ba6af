#!/usr/bin/env python3
"""What finishing the PNG files on the device (api.png_file / srx_png_file_*: srx_png_deflate_*'s stream, its CRC-32 and the container) costs
beside wrapping the device's streams on the host (session.png_container), with the protocol of tools/png_time.py:

  * device time of srx_png_file_f32 and of srx_png_deflate_f32 on the same [3, 3072, 4096] and [3, 1536, 2048] float planes in one process,
    and of srx_crc32 alone on the streams: HIP events around the call, the best and the median of --iters calls after --warmup, --rounds
    rounds; the spread is that of the rounds' bests;
  * host time per file of a writer job on one thread, best of --host-iters, in two forms -- the parent's (tobytes + png_container + write)
    and write(memoryview) of the device-made file -- each to a file in a temporary directory and to /dev/null;
  * tools/png_time.py's session_e2e workload (2 mono_barcodes sessions x 4 reps of 768 x 1024 frames, files to files, device_png on) with
    session.DEVICE_PNG_FILES off (the parent's job form) and on, alternating in one process, --e2e-rounds rounds.  The session takes the
    file form if no round of it is slower than the slowest round of the parent's form (`file_form_not_slower`).

usage: tools/png_file_time.py [--iters N] [--warmup N] [--rounds N] [--host-iters N] [--e2e-rounds N] [--no-e2e] [--json PATH]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sr_mi355x as S  # noqa: E402
from sr_mi355x import api, session, synth  # noqa: E402
from png_time import SHAPES, event_us, planes  # noqa: E402


def best_ms(fn, iters):
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(min(t)), t


def rows_of(a):
    rows = []
    lib = api._lib.load()
    for B, H, W in SHAPES:
        x = torch.from_numpy(planes(B, H, W)).to("cuda", torch.float32)
        streams = torch.empty((B, lib.srx_png_stream_bound(H, W)), dtype=torch.uint8, device="cuda")
        files = torch.empty((B, lib.srx_png_file_bound(H, W)), dtype=torch.uint8, device="cuda")
        lengths = torch.empty((B,), dtype=torch.int64, device="cuda")
        flengths = torch.empty((B,), dtype=torch.int64, device="cuda")
        crc = torch.empty((B,), dtype=torch.int32, device="cuda")
        ws, wsp, wsn = api._ws(max(lib.srx_png_file_scratch_bytes(B, H, W), lib.srx_crc32_scratch_bytes(B, streams.shape[1])))
        st = api._stream()
        deflate = lambda: api._lib.check(lib.srx_png_deflate_f32(api._p(x), B, H, W, api._p(streams), api._p(lengths), wsp, wsn, st), "deflate")  # noqa: E731
        whole = lambda: api._lib.check(lib.srx_png_file_f32(api._p(x), B, H, W, api._p(files), api._p(flengths), wsp, wsn, st), "file")  # noqa: E731
        crc_only = lambda: api._lib.check(lib.srx_crc32(api._p(streams), B, streams.shape[1], streams.shape[1], api._p(lengths), 0, api._p(crc),  # noqa: E731
                                                        wsp, wsn, st), "crc32")
        deflate()
        t = {"deflate": [], "file": [], "crc32": []}
        for _ in range(a.rounds):  # alternating within a round
            for name, fn in (("deflate", deflate), ("file", whole), ("crc32", crc_only)):
                t[name].append(event_us(fn, a.iters, a.warmup))
        n, fn_ = lengths.cpu().tolist(), flengths.cpu().tolist()
        hs, hf = streams.cpu(), files.cpu()
        for b in range(B):  # what is timed is also right
            z = hs[b, :n[b]].numpy().tobytes()
            assert hf[b, :fn_[b]].numpy().tobytes() == session.png_container(W, H, z)
            assert (int(crc[b]) & 0xFFFFFFFF) == zlib.crc32(z)
        # a writer job, one thread: pinned slots as the session holds them
        ps, pf = hs.pin_memory(), hf.pin_memory()
        host = {}
        with tempfile.TemporaryDirectory() as d:
            for where, path in (("file", os.path.join(d, "{b}.png")), ("devnull", os.devnull)):
                def parent_form():
                    for b in range(B):
                        with open(path.format(b=b), "wb") as fp:
                            fp.write(session.png_container(W, H, ps[b, :n[b]].numpy().tobytes()))

                def file_form():
                    for b in range(B):
                        with open(path.format(b=b), "wb") as fp:
                            fp.write(memoryview(pf[b, :fn_[b]].numpy()))

                for name, fn in (("parent", parent_form), ("memoryview", file_form)):
                    best, all_ = best_ms(fn, a.host_iters)
                    host[f"ms_per_file_{name}_{where}"] = best / B
                    host[f"ms_per_file_{name}_{where}_all"] = [v / B for v in all_]
        r = dict(B=B, H=H, W=W, stream_bytes=n, scratch_bytes=int(wsn.value))
        for name in t:
            best, med = zip(*t[name])
            r[f"us_{name}_best"] = float(min(best))
            r[f"us_{name}_best_rounds"] = list(best)
            r[f"us_{name}_median_rounds"] = list(med)
            r[f"spread_{name}_best"] = (max(best) - min(best)) / min(best)
        r["us_file_minus_deflate"] = r["us_file_best"] - r["us_deflate_best"]
        r.update(host)
        rows.append(r)
        del x, streams, files, ws
        torch.cuda.empty_cache()
    return rows


def e2e_leg(rounds, n_sessions=2, reps=4, lr_hw=(768, 1024)):
    """tools/png_time.py's session_e2e workload with device_png on, once per round in the parent's job form and in the file form"""
    from PIL import Image
    h, w = lr_hw
    tmp = tempfile.mkdtemp(prefix="srx_png_file_e2e_")
    keep = session.DEVICE_PNG_FILES
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
        for form in (False, True):
            session.DEVICE_PNG_FILES = form
            session.process_sessions(sessions[:1], psf, os.path.join(tmp, f"warm{int(form)}"), "mono_barcodes", verbose=False, device_png=True)
        for rnd in range(rounds):
            for form in (False, True):
                session.DEVICE_PNG_FILES = form
                out = os.path.join(tmp, f"out{rnd}_{int(form)}")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                written = session.process_sessions(sessions, psf, out, "mono_barcodes", verbose=False, device_png=True)
                torch.cuda.synchronize()
                t[form].append((time.perf_counter() - t0) / len(written) * 1e3)
                shutil.rmtree(out, ignore_errors=True)
        return dict(workload=f"{n_sessions} mono_barcodes sessions x {reps} reps, {h}x{w} frames, 80 IBP iterations, files to files, device_png",
                    host_threads=session._host_threads(), rounds=rounds, ms_per_rep_parent_form_rounds=t[False], ms_per_rep_file_form_rounds=t[True],
                    ms_per_rep_parent_form=float(np.median(t[False])), ms_per_rep_file_form=float(np.median(t[True])),
                    parent_over_file=float(np.median(t[False]) / np.median(t[True])),
                    file_form_not_slower=bool(max(t[True]) <= max(t[False])), file_form_faster_beyond_spread=bool(max(t[True]) < min(t[False])))
    finally:
        session.DEVICE_PNG_FILES = keep
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--e2e-rounds", type=int, default=3)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("png_file_time.py needs a GPU")
    rows = rows_of(a)
    for r in rows:
        print(f"[{r['B']}, {r['H']}, {r['W']}] float32: srx_png_file {r['us_file_best']:.0f} us, srx_png_deflate {r['us_deflate_best']:.0f} us "
              f"(bests; spreads {100 * r['spread_file_best']:.1f} % and {100 * r['spread_deflate_best']:.1f} %), srx_crc32 on the streams "
              f"{r['us_crc32_best']:.0f} us; a writer job per file: {r['ms_per_file_parent_file']:.2f} ms in the parent's form, "
              f"{r['ms_per_file_memoryview_file']:.2f} ms as write(memoryview) ({r['ms_per_file_parent_devnull']:.2f} and "
              f"{r['ms_per_file_memoryview_devnull']:.2f} ms to /dev/null)")
    e2e = None if a.no_e2e else e2e_leg(a.e2e_rounds)
    if e2e:
        print(f"session_e2e with device_png: {e2e['ms_per_rep_parent_form']:.2f} ms per rep in the parent's job form, {e2e['ms_per_rep_file_form']:.2f} ms "
              f"in the file form ({e2e['parent_over_file']:.3f} x; file form not slower than the parent's slowest round: {e2e['file_form_not_slower']}), "
              f"{e2e['host_threads']} host threads")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup, rounds=a.rounds, rows=rows, session_e2e=e2e), f, indent=1)


if __name__ == "__main__":
    main()
