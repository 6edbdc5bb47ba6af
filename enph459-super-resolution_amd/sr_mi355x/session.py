"""Session driver: the counterpart of the reference's `process_session` / `process_combo` on the device path.

Reproduces, for the four experiment layouts of the reference, the file discovery rules, frame order, shift
tables, outputs and `done.flag` skip logic:

  kind            reference                                 input files                         LR frames
  --------------  ----------------------------------------  ----------------------------------  -----------------------------
  mono_cal_target mono_cal_target/run_sr.py:59-99,262-315   center.png, shift_0..3.png          5, nominal (0,0), (+-.5,+-.5)
  rgb_cal_target  rgb_cal_target/run_sr.py:63-113,276-333   corner{c}_rep{rr}.png+metadata.json 4 = red plane, mean over reps,
                                                                                                shifts = expected px / 2
  mono_barcodes   mono_barcodes/run_sr.py:71-130,293-351    corner{c}_rep{rr}.png               4 per rep, nominal +-0.5
  rgb_barcodes    rgb_barcodes/run_sr.py:78-143,306-364     corner{c}_rep{rr}.png               4 per rep (red), nominal +-0.5

PNG decode/encode stays on the host (PIL), everything between -- uint8 -> float, Bayer red extraction, rep
averaging, frame mean, Native-2x zoom, shift_and_add, ibp, clip+truncate to uint8 -- runs in libsrx on the GPU.
The reference's matplotlib figures (comparison.png, convergence.png) are not produced; the IBP MSE trace is
written as `convergence.json` instead.

register=True (run_sr --register) measures the shifts from the loaded frames (sr_mi355x.register.estimate_shifts, with the
table above as init and anchor: one item per rep for the barcode kinds, the rep-averaged red planes for rgb_cal_target) and
reconstructs with them (uint8 frames, keep_u8, are measured as bytes); frames whose estimate has a nonzero status keep their table shift.  registration.json records the table,
the estimates, the shifts used, the scores and the status codes.  Without it, nothing differs.

colour=True (run_sr --colour; the two rgb_* kinds) reconstructs all four Bayer planes of the raw frames as one batch under the one table
(reconstruct_colour) and writes native_2x_rgb.png, SAA_rgb.png, SAA_IBP_rgb.png and convergence_planes.json beside the files above, which
keep their bytes: the reference's grey images of the red plane stay the default.
"""
import json
import os
import re

import numpy as np

from . import api

UPSAMPLE_FACTOR = 2
PSF_SIZE, PSF_SIGMA, PSF_HALFWIDTH = 7, 1.0, 3
IBP_STEP_SIZE = 0.5
IBP_ITERATIONS = {"mono_cal_target": 80, "rgb_cal_target": 50, "mono_barcodes": 80, "rgb_barcodes": 80}

# mono_cal_target/run_sr.py:59-66
IMAGE_SHIFTS = [("center.png", (0.0, 0.0)), ("shift_0.png", (+0.5, -0.5)), ("shift_1.png", (+0.5, +0.5)),
                ("shift_2.png", (-0.5, -0.5)), ("shift_3.png", (-0.5, +0.5))]
# mono_barcodes/run_sr.py:71-76, rgb_barcodes/run_sr.py:78-83 (corner0..3)
CORNER_SHIFTS = [(+0.5, -0.5), (+0.5, +0.5), (-0.5, -0.5), (-0.5, +0.5)]
# rgb_cal_target/run_sr.py:63
CORNER_ORDER = ["(-x,+y)", "(+x,+y)", "(-x,-y)", "(+x,-y)"]


def _png_u8(path):
    from PIL import Image
    a = np.array(Image.open(path))
    if a.ndim == 3:  # load_gray: channel mean (run_sr.py:73-75)
        return a.astype(np.float64).mean(axis=2)
    return a


LOADER_PRECISION = "f64"  # uint8 -> float, Bayer extraction and the rep / frame means are done in the reference's
#                           own float64 (exact for uint8 data), whatever precision the SR kernels then run in: a mean
#                           of k/5 values rounded to float32 flips the truncating uint8 quantiser on ~0.5 % of pixels.


def _loader_precision():
    """The loaders' arithmetic in LOADER_PRECISION on the calling thread only (the Prefetcher's thread decodes the next session
    while the main thread reconstructs the current one in its own precision)."""
    return api.precision_override(LOADER_PRECISION)


_decoders = None


def _decode_many(paths):
    """The PNG files of one session decoded side by side (PIL releases the GIL while it inflates): a 16-frame barcode session
    spent 80 ms in this loop, one file after the other."""
    global _decoders
    if _decoders is None:
        import concurrent.futures
        _decoders = concurrent.futures.ThreadPoolExecutor(max_workers=_host_threads())
    return list(_decoders.map(_png_u8, paths))


def _to_dev_f(a):
    if a.dtype == np.uint8:
        return api.u8_to_float(a, precision=LOADER_PRECISION)
    return api._to_dev(a, LOADER_PRECISION)[0]


def _to_dev_frames(decoded, keep_u8):
    """The decoded files of one frame set on the device: float64 (load_gray's cast), or -- keep_u8, and every file 8-bit greyscale -- the
    bytes as they are (a quarter of the upload of float32 frames, an eighth of these; shift_and_add and ibp take them through
    srx_saa_u8lr / srx_ibp_u8lr, registration through srx_register_u8).  A colour file (load_gray's channel mean is not an integer) keeps the whole set in float64."""
    if keep_u8 and api._is_u8(decoded):
        return [api._to_dev(a)[0] for a in decoded]
    return [_to_dev_f(a) for a in decoded]


def _frame_mean(lr):
    """np.mean over the frames of [B, N, h, w] in LOADER_PRECISION -> [B, h, w]: float64 stacks through mean_frames_batched, uint8 stacks
    (keep_u8 loaders) as bytes through mean_u8 (the same bits, no float copy of the frames)"""
    import torch
    if lr.dtype == torch.uint8:
        return api.mean_u8(lr, precision=LOADER_PRECISION)
    with _loader_precision():
        return api.mean_frames_batched(lr)


def load_gray_dev(path, decoded=None):
    """PNG -> float64 image on the device (load_gray, mono_cal_target/run_sr.py:73-75).  decoded: the file's pixels, if a caller
    already has them (_decode_many)."""
    return _to_dev_f(_png_u8(path) if decoded is None else decoded)


def detect_kind(session_dir):
    names = os.listdir(session_dir)
    if "center.png" in names:
        return "mono_cal_target"
    if any(re.match(r"corner\d+_rep\d+\.png", n) for n in names):
        return None  # caller must say which of the three corner layouts it is
    raise FileNotFoundError(f"no SR input images in {session_dir}")


def load_mono_cal_session(session_dir, keep_u8=False):
    """mono_cal_target/run_sr.py:78-99 -> (frames on device, shifts).  keep_u8: the frames stay uint8 (_to_dev_frames)."""
    present = [(os.path.join(session_dir, fname), s) for fname, s in IMAGE_SHIFTS if os.path.exists(os.path.join(session_dir, fname))]
    frames = _to_dev_frames(_decode_many([p for p, _ in present]), keep_u8)
    shifts = [s for _, s in present]
    if len(frames) < 2:
        raise FileNotFoundError(f"Need at least 2 images in {session_dir}")
    return frames, shifts


def load_rgb_cal_combo(combo_dir, keep_u8=False, planes="red"):
    """rgb_cal_target/run_sr.py:78-113: red plane of every rep, mean over reps, shifts = metadata px / 2.
    planes="all": every corner's frame is the [4, h, w] stack of its four Bayer planes (R, G1, G2, B; api.bayer_split / bayer_mean_u8: the
    raw frames are read once); plane 0 is the red frame of the default, bit for bit.
    keep_u8, and every file 8-bit greyscale: the reps go up as bytes and mean_u8(f=2) forms each corner's frame from them -- the four
    corners in one call when they have the same number of reps -- which is the same float64 frame, bit for bit.  A colour file (load_gray's
    channel mean is not an integer) keeps the whole combo on the float64 path, as in load_corner_reps."""
    import torch
    with open(os.path.join(combo_dir, "metadata.json")) as fp:
        meta = json.load(fp)

    def get_shift(label):
        if "expected_shifts" in meta:
            s = meta["expected_shifts"][label]
            return s["dy_px"] / 2.0, s["dx_px"] / 2.0
        if "corners" in meta:
            c = meta["corners"][label]
            return c["expected_dy_px"] / 2.0, c["expected_dx_px"] / 2.0
        raise KeyError(f"Cannot find shift for {label} in metadata")

    counts, paths, shifts = [], [], []
    for idx, label in enumerate(CORNER_ORDER):
        reps = sorted(f for f in os.listdir(combo_dir) if f.startswith(f"corner{idx}_rep") and f.endswith(".png"))
        if not reps:
            raise FileNotFoundError(f"No images for corner{idx} in {combo_dir}")
        counts.append(len(reps))
        paths += [os.path.join(combo_dir, r) for r in reps]
        shifts.append(get_shift(label))
    decoded = _decode_many(paths)
    starts = np.concatenate([[0], np.cumsum(counts)])
    corners = [decoded[starts[k]:starts[k + 1]] for k in range(len(counts))]
    if planes not in ("red", "all"):
        raise ValueError("planes must be 'red' or 'all'")
    if keep_u8 and api._is_u8(decoded):
        def mean_u8(x):  # [B, R, H, W] bytes -> the B frames
            return api.bayer_mean_u8(x, precision=LOADER_PRECISION) if planes == "all" else api.mean_u8(x, f=2, precision=LOADER_PRECISION)

        def reps_dev(groups):  # [len(groups), R, H, W] on the device, every file uploaded as its own bytes
            files = _to_dev_frames([a for group in groups for a in group], True)
            return torch.stack(files).reshape((len(groups), len(groups[0])) + files[0].shape)

        if len(set(counts)) == 1:  # one B = 4 call
            return list(mean_u8(reps_dev(corners))), shifts
        return [mean_u8(reps_dev([c]))[0] for c in corners], shifts
    cut = api.bayer_split if planes == "all" else api.extract_red
    frames = []
    with _loader_precision():
        for c in corners:
            frames.append(api.mean_frames([cut(_to_dev_f(a)) for a in c]))
    return frames, shifts


def load_corner_reps(session_dir, red, keep_u8=False):
    """mono_barcodes/run_sr.py:89-130 / rgb_barcodes/run_sr.py:102-143 -> (list over reps of 4 frames, shifts).
    keep_u8: the frames stay uint8 (_to_dev_frames); the red plane is then cut out of the bytes (extract_red_u8).
    red="all": every frame is the [4, h, w] stack of its four Bayer planes (api.bayer_split, on the bytes under keep_u8); plane 0 is the
    red frame of red=True."""
    rep_indices = sorted({int(m.group(1)) for m in (re.match(r"corner\d+_rep(\d+)\.png", n) for n in os.listdir(session_dir))
                          if m})
    if not rep_indices:
        raise FileNotFoundError(f"No corner*_rep*.png files in {session_dir}")
    paths = [os.path.join(session_dir, f"corner{ci}_rep{ri:02d}.png") for ri in rep_indices for ci in range(4)]
    for path in paths:
        if not os.path.exists(path):
            raise FileNotFoundError(f"Missing {path}")
    decoded = _decode_many(paths)
    keep_u8 = keep_u8 and api._is_u8(decoded)  # (one colour file: the whole session in float64, as without the switch)
    all_reps = []
    for k in range(len(rep_indices)):
        frames = []
        for img in _to_dev_frames(decoded[4 * k:4 * k + 4], keep_u8):
            if keep_u8:
                frames.append(api.bayer_split(img) if red == "all" else api.extract_red_u8(img) if red else img)
                continue
            with _loader_precision():
                frames.append(api.bayer_split(img) if red == "all" else api.extract_red(img) if red else img)
        all_reps.append(frames)
    return all_reps, list(CORNER_SHIFTS)


def reconstruct(frames, shifts, psf_kernel, n_iter, factor=UPSAMPLE_FACTOR, step=IBP_STEP_SIZE, row_bands=False, patchwise=None,
                patch_opts=None):
    """Native-2x, SAA and SAA+IBP of one frame set, all on the device (run_sr.py:274-292).
    -> dict of float device tensors + the MSE trace.
    row_bands: every rank of the process group calls this with the same frames; the IBP loop runs on row bands of the ONE image
    (rowband.ibp_row_bands: halo rows exchanged point to point), and only rank 0 gets "SAA_IBP" (None elsewhere).
    patchwise: None (the whole frame under the one table, as the reference), "global" (cut into overlapping patches, every patch
    under the one table, blended back) or "local" (every patch under the shifts registered on it): patchwise.reconstruct_patchwise
    with PatchGrid(h, w, factor, **patch_opts).  The dict then also holds "shift_field" (shift_field.json's content; "local" only)."""
    import torch
    if patchwise is not None:
        from . import patchwise as pw
        if patchwise not in ("global", "local"):
            raise ValueError("patchwise must be None, 'global' or 'local'")
        if row_bands:
            raise ValueError("patchwise and row_bands exclude each other")
        h, w = (int(v) for v in frames[0].shape)
        grid = pw.PatchGrid(h, w, factor, **(patch_opts or {}))
        images, errs, field = pw.reconstruct_patchwise(frames, shifts, psf_kernel, n_iter, factor, step, grid=grid, local=patchwise == "local")
        if field is not None:
            images["shift_field"] = pw.field_json(grid, shifts, field)
        return images, errs
    lr64 = torch.stack(frames)  # float64, or uint8 frames (keep_u8 loaders): SAA and IBP then take the bytes themselves
    u8 = lr64.dtype == torch.uint8
    mean_lr = _frame_mean(lr64[None])[0]  # float64; also what LR_(red_)mean.png is quantised from
    native = api.zoom_batched(mean_lr[None], factor)[0]
    if u8 and not row_bands:
        saa = api.shift_and_add_u8_batched(lr64[None], shifts, factor)
        hr, errs = api.ibp_u8_batched(lr64[None], shifts, psf_kernel, saa.clone(), factor, n_iter, step)
        return {"native_2x": native, "SAA": saa[0], "SAA_IBP": hr[0], "LR_mean": mean_lr}, [float(e) for e in errs[0].cpu()]
    lr = api.u8_to_float(lr64) if u8 else lr64.to(api._TORCH_DT[api.get_precision()])  # (row bands run on plans: float frames)
    saa = api.shift_and_add_batched(lr[None], shifts, factor)
    if row_bands:
        from . import rowband
        import torch.distributed as dist
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        m = 2  # two iterations per halo exchange (half the messages) where the bands are tall enough for the doubled halo
        try:
            rowband.band_plan(lr.shape[1], factor, world, m * rowband.reach_rows(factor, shifts, np.asarray(psf_kernel).shape[0], api.get_precision()))
        except ValueError:
            m = 1
        band, errs, bounds = rowband.ibp_row_bands(lr, shifts, psf_kernel, saa[0], factor, n_iter, step, precision=api.get_precision(),
                                                   iters_per_exchange=m)
        full = rowband.gather_rows(band, bounds, saa.shape[1])
        hr0 = None if full is None else torch.from_numpy(full).to(saa)
        return {"native_2x": native, "SAA": saa[0], "SAA_IBP": hr0, "LR_mean": mean_lr}, errs
    hr, errs = api.ibp_batched(lr[None], shifts, psf_kernel, saa.clone(), factor, n_iter, step)
    return {"native_2x": native, "SAA": saa[0], "SAA_IBP": hr[0], "LR_mean": mean_lr}, [float(e) for e in errs[0].cpu()]


def register_shifts(frame_sets, shifts):
    """register=True: estimate_shifts on B frame sets of one shape (a batch of B items) with the table as init and anchor.
    -> one (shifts used, registration.json content) per frame set; a frame with a nonzero status keeps its table shift.
    uint8 frame sets (keep_u8 loaders) are registered as bytes (srx_register_u8: the same bits, no float copy of the frames); float sets
    (rgb_cal_target's rep-averaged planes) go on as they are."""
    import torch
    from . import register
    table = np.asarray(shifts, dtype=np.float64)
    lr = torch.stack([torch.stack(list(fr)) for fr in frame_sets])  # float64, or uint8 (keep_u8 loaders): registered as bytes, the same bits
    est, score, status = register.estimate_shifts(lr, init=table, full=True)
    out = []
    for b in range(len(frame_sets)):
        used = np.where((status[b] == 0)[:, None], est[b], table)
        out.append(([tuple(float(v) for v in s) for s in used],
                    {"nominal": table.tolist(), "estimated": est[b].tolist(), "used": used.tolist(), "score": score[b].tolist(),
                     "status": status[b].tolist()}))
    return out


def reconstruct_batch(frame_sets, shifts, psf_kernel, n_iter, factor=UPSAMPLE_FACTOR, step=IBP_STEP_SIZE, lazy_errors=False):
    """`reconstruct` for B frame sets of one shape and one shift table in ONE library call per stage (B = the reps of a
    barcode session, mono_barcodes/run_sr.py:301-351: independent work items).  Every item's result is bit-identical to
    reconstruct() on that item alone (the kernels treat batch entries independently; tests/test_gpu_session.py).
    shifts: one table [N, 2] for every frame set, or a list of B tables (register=True measures one per rep): still one call per
    stage, through the library's per-item entry points (srx_saa_items_* / srx_ibp_items_*), every item as on its own.
    -> list of (images dict, MSE trace), one per frame set.  lazy_errors: the traces stay device tensors (no wait for the IBP loop
    here; _save_outputs downloads them with the planes)."""
    import torch
    lr64 = torch.stack([torch.stack(fr) for fr in frame_sets])  # [B, N, h, w] float64, or uint8 (keep_u8 loaders)
    B, N, h, w = lr64.shape
    shifts = np.asarray(shifts, dtype=np.float64)
    if shifts.shape not in ((N, 2), (B, N, 2)):
        raise ValueError(f"shifts must be one table {(N, 2)} or one per frame set {(B, N, 2)}, not {shifts.shape}")
    mean_lr = _frame_mean(lr64)
    native = api.zoom_batched(mean_lr, factor)
    if lr64.dtype == torch.uint8:
        saa = api.shift_and_add_u8_batched(lr64, shifts, factor)
        hr, errs = api.ibp_u8_batched(lr64, shifts, psf_kernel, saa.clone(), factor, n_iter, step)
    else:
        lr = lr64.to(api._TORCH_DT[api.get_precision()])
        saa = api.shift_and_add_batched(lr, shifts, factor)
        hr, errs = api.ibp_batched(lr, shifts, psf_kernel, saa.clone(), factor, n_iter, step)
    if not lazy_errors:
        errs = errs.cpu()
    return [({"native_2x": native[i], "SAA": saa[i], "SAA_IBP": hr[i], "LR_mean": mean_lr[i]}, errs[i] if lazy_errors else [float(e) for e in errs[i]])
            for i in range(B)]


HR_NAMES = ("native_2x", "SAA", "SAA_IBP")


def reconstruct_colour_batch(rep_frames, shifts, psf_kernel, n_iter, factor=UPSAMPLE_FACTOR, step=IBP_STEP_SIZE, gains=None):
    """The colour reconstruction of B frame sets (the reps of an rgb_barcodes session): every set is N frames of [4, h, w] Bayer planes
    (load_corner_reps(red="all")), and the B x 4 planes go through reconstruct_batch as ONE batch -- one library call per stage, uint8 stacks
    through the u8lr calls -- under the one table, or under one table per set (shifts [B, N, 2]: every set's four planes share its table;
    all four planes have the same pitch).  Item 4 b of the batch is the red reconstruction of set b, what reconstruct gives for its red
    frames.  native_2x, SAA and SAA_IBP are then laid over each other (api.bayer_merge at `factor`, rgb8).
    -> per set (the RGB byte images {name: uint8 [H, W, 3]}, the four per-plane image dicts, the four MSE traces)."""
    import torch
    B = len(rep_frames)
    sets = [[fr[p] for fr in frames] for frames in rep_frames for p in range(4)]
    table = np.asarray(shifts, dtype=np.float64)
    if table.ndim == 3:
        table = np.repeat(table, 4, axis=0)
    results = reconstruct_batch(sets, table, psf_kernel, n_iter, factor, step)
    out = []
    for b in range(B):
        mine = results[4 * b:4 * b + 4]
        stacks = torch.stack([torch.stack([images[name] for images, _ in mine]) for name in HR_NAMES])  # [3 names, 4 planes, H, W]
        rgb = api.bayer_merge(stacks, factor, gains, rgb8=True)
        out.append(({name: rgb[k] for k, name in enumerate(HR_NAMES)}, [images for images, _ in mine], [trace for _, trace in mine]))
    return out


def reconstruct_colour(plane_frames, shifts, psf_kernel, n_iter, factor=UPSAMPLE_FACTOR, step=IBP_STEP_SIZE, gains=None):
    """reconstruct_colour_batch for one frame set: the N frames of [4, h, w] as a batch of four items under the one table.
    -> (RGB byte images, the four per-plane image dicts, the four MSE traces); item 0 is the red reconstruction."""
    return reconstruct_colour_batch([plane_frames], shifts, psf_kernel, n_iter, factor, step, gains)[0]


class Prefetcher:
    """Host work of items k + 1 .. k + depth (PNG decode, uint8 -> device) overlapped with the device work of item k: worker threads run
    `load(item)` for the next items while the caller consumes the current one.  PIL releases the GIL while it inflates a PNG,
    and the host-to-device copies it issues go to the thread's own stream, so neither blocks the compute stream."""

    def __init__(self, items, load, depth=2):
        import collections
        import concurrent.futures
        self._items, self._load, self._depth = list(items), load, max(1, depth)
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=self._depth)  # `depth` items ahead, one loader thread each
        self._queue = collections.deque(self._pool.submit(self._guarded, it) for it in self._items[:self._depth])

    def _guarded(self, item):
        import torch
        if torch.cuda.is_available():
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                out = self._load(item)
            stream.synchronize()
            return out
        return self._load(item)

    @staticmethod
    def _adopt(obj):
        """The tensors were allocated under the loader's side stream and are consumed on the caller's: tell the caching allocator,
        so that a block freed by the consumer is not handed to the next prefetch while the compute stream still reads it."""
        import torch
        if isinstance(obj, torch.Tensor):
            if obj.is_cuda:
                obj.record_stream(torch.cuda.current_stream())
        elif isinstance(obj, (list, tuple)):
            for o in obj:
                Prefetcher._adopt(o)

    def __iter__(self):
        try:
            for k, item in enumerate(self._items):
                cur = self._queue.popleft().result()
                if k + self._depth < len(self._items):
                    self._queue.append(self._pool.submit(self._guarded, self._items[k + self._depth]))
                self._adopt(cur)
                yield item, cur
        finally:  # also when the consumer raises or stops early
            self._pool.shutdown(wait=True, cancel_futures=True)


def _host_threads():
    """Threads for the PNG decode / encode pools: the cores this process may run on (a one-GPU share of a node is 16), at most 16 --
    zlib and PIL release the GIL, and the files-to-files rate is bounded by exactly this work."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 1
    return max(1, min(16, n))


DEVICE_PNG_FILES = True  # device_png: whole files from the device (api.png_file); False: its streams, wrapped by png_container in the jobs
PNG_COMPRESS_LEVEL = 1  # zlib level of the PNGs written (PIL's default is 6: ~4x the encode time for ~10 % smaller files; lossless either way)
_writers, _pending = None, []


def write_png_u8(path, arr):
    """An 8-bit greyscale PNG of a 2-D uint8 array (what cv2.imwrite / PIL write for the reference's outputs, mono_barcodes/run_sr.py:
    303-306; the same pixels back from any reader).  PIL's encoder tries the five scanline filters on every row and spent 55 ms on a
    1536 x 2048 plane -- the files-to-files rate of a session is exactly this work.  Here: the Up filter on the whole image as one
    numpy subtraction and one zlib pass with run-length matching only (Z_RLE: on Up-filtered reconstructions within 8 % of PIL's file
    size at level 1, in 0.4x its time -- measured on the reference's committed 3072 x 4096 SAA.png: 118 against 298 ms)."""
    a = np.ascontiguousarray(arr)
    if a.ndim != 2 or a.dtype != np.uint8:
        from PIL import Image
        Image.fromarray(a).save(path, compress_level=PNG_COMPRESS_LEVEL)
        return
    h, w = a.shape
    with open(path, "wb") as fp:
        fp.write(png_container(w, h, _up_filtered_stream(a)))


def _up_filtered_stream(a):
    """the zlib stream of the Up-filtered scanlines of a 2-D uint8 array (write_png_u8's and write_png_rgb8's IDAT data)"""
    import zlib
    h, w = a.shape
    raw = np.empty((h, w + 1), np.uint8)
    raw[:, 0] = 2          # filter type of every scanline: Up
    raw[0, 1:] = a[0]      # (the row above the first is zero)
    np.subtract(a[1:], a[:-1], out=raw[1:, 1:])  # modulo 256
    c = zlib.compressobj(PNG_COMPRESS_LEVEL, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return c.compress(raw) + c.flush()


def write_png_rgb8(path, arr):
    """An 8-bit truecolour PNG of a uint8 [H, W, 3] array, write_png_u8's way: under the Up filter the scanlines are those of the grey
    image [H, 3 W], in the container api.png_file_rgb8 builds on the device (colour type 2)."""
    a = np.ascontiguousarray(arr)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("write_png_rgb8 needs a uint8 [H, W, 3] array")
    h, w = a.shape[:2]
    with open(path, "wb") as fp:
        fp.write(png_container(w, h, _up_filtered_stream(a.reshape(h, 3 * w)), colour_type=2))


def png_container(w, h, zstream, colour_type=0):
    """The bytes of an 8-bit greyscale (or, colour_type=2, truecolour) PNG file around the zlib stream of its scanlines: signature, IHDR, one IDAT, IEND.  The stream is
    write_png_u8's own or the device's (api.png_deflate); the chunks' CRC-32 is host work either way (zlib.crc32 releases the GIL and
    takes a few ms on the few MB of a 3072 x 4096 plane)."""
    import struct
    import zlib

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)) & 0xffffffff)

    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)) + chunk(b"IDAT", bytes(zstream)) + chunk(b"IEND", b"")


def _writer_pool():
    global _writers
    if _writers is None:
        import concurrent.futures
        _writers = concurrent.futures.ThreadPoolExecutor(max_workers=_host_threads())
    return _writers


def flush_writes():
    """Wait for the PNG encodes queued by _save_outputs (they run on worker threads: zlib releases the GIL)."""
    global _pending
    pend, _pending = _pending, []
    for f in pend:
        f.result()


def _save_outputs(out_dir, images, errors, lr_name, extra=None, device_png=False, rgb=None):
    """Quantise on the device (clip + truncate, run_sr.py:303), queue the copies of the uint8 planes into pinned host buffers and hand
    the PNG encoding to worker threads, which wait for the copies' event -- the calling thread waits for nothing and goes on to queue the
    next item's device work.  `errors`: the MSE trace, a list or a device tensor (downloaded with the planes).  done.flag is written by
    the last job of the directory, after every file of it exists.
    device_png: the device compresses as well (same pixels in the files, other bytes) and, with DEVICE_PNG_FILES, builds the container and
    its CRC-32 around the stream (api.png_file): a job writes its slot's bytes as they are.  With DEVICE_PNG_FILES off the device makes the
    streams only (api.png_deflate) and the jobs wrap them (png_container: the CRC-32 on the host) -- the same files byte for byte.
    rgb: {name: uint8 [H, W, 3]} (reconstruct_colour) -> {name}_rgb.png beside the grey files: whole files from api.png_file_rgb8 under
    device_png, write_png_rgb8 otherwise."""
    import torch
    os.makedirs(out_dir, exist_ok=True)

    def to_host(t):
        if not t.is_cuda:
            return t
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        return h

    hr_names = HR_NAMES
    if device_png:
        # the three HR planes as one [3, H, W] call on the float tensors (quantised as they are read), LR_mean as a second one in the
        # loader's precision; what goes to the host is the slots and their lengths, and a job slices and writes
        files = DEVICE_PNG_FILES
        encode = api.png_file if files else api.png_deflate
        hr = torch.stack([images[name] for name in hr_names])
        streams, lengths = encode(hr)
        with _loader_precision():
            lr_streams, lr_lengths = encode(images["LR_mean"])
        hr_host, hr_len, lr_host, lr_len = to_host(streams), to_host(lengths), to_host(lr_streams), to_host(lr_lengths)
        planes = {f"{name}.png": (hr_host, hr_len, k, tuple(hr.shape[1:]), files) for k, name in enumerate(hr_names)}
        planes[lr_name] = (lr_host, lr_len, 0, tuple(images["LR_mean"].shape), files)
        if rgb:
            rgb_files, rgb_lengths = api.png_file_rgb8(torch.stack([rgb[name] for name in hr_names]))
            rgb_host, rgb_len = to_host(rgb_files), to_host(rgb_lengths)
            planes.update({f"{name}_rgb.png": (rgb_host, rgb_len, k, tuple(rgb[name].shape[:2]), True) for k, name in enumerate(hr_names)})
    else:
        planes = {f"{name}.png": to_host(api.quantize_u8(images[name])) for name in hr_names}
        with _loader_precision():
            planes[lr_name] = to_host(api.quantize_u8(images["LR_mean"]))
        if rgb:
            planes.update({f"{name}_rgb.png": to_host(rgb[name]) for name in hr_names})
    err_host = to_host(errors) if isinstance(errors, torch.Tensor) else None
    ready = None
    if torch.cuda.is_available():
        ready = torch.cuda.Event()
        ready.record()

    # one job per FILE (a rep's four PNGs used to be one job: 3 x 55 ms of zlib in a row while other threads idled -- 177 ms until a
    # session's files were out, with 4.5 ms of device work behind them); the job that finishes last writes the side files and done.flag
    import threading
    left, lock = [len(planes)], threading.Lock()

    def finish():
        trace = errors if err_host is None else [float(e) for e in err_host]
        with open(os.path.join(out_dir, "convergence.json"), "w") as fp:
            json.dump({"ibp_mse": trace}, fp)
        if extra:
            for fname, obj in extra.items():
                with open(os.path.join(out_dir, fname), "w") as fp:
                    json.dump(obj, fp, indent=2)
        open(os.path.join(out_dir, "done.flag"), "w").close()

    def job(fname, host):
        if ready is not None:
            ready.synchronize()
        if device_png:
            slots, lens, k, (h, w), whole = host
            with open(os.path.join(out_dir, fname), "wb") as fp:
                if whole:
                    fp.write(memoryview(slots[k, :int(lens[k])].numpy()))
                else:
                    fp.write(png_container(w, h, slots[k, :int(lens[k])].numpy().tobytes()))
        elif host.dim() == 3:
            write_png_rgb8(os.path.join(out_dir, fname), host.numpy())
        else:
            write_png_u8(os.path.join(out_dir, fname), host.numpy())
        with lock:
            left[0] -= 1
            last = left[0] == 0
        if last:
            finish()

    for fname, host in planes.items():
        _pending.append(_writer_pool().submit(job, fname, host))


def process_session(session_dir, psf_kernel, output_base, kind=None, n_iter=None, verbose=True, batch_reps=True, loaded=None, flush=True,
                    row_bands=False, on_images=None, register=False, keep_u8=False, device_png=False, patchwise=None, patch_opts=None,
                    colour=False):
    """Counterpart of process_session / process_combo.  Returns the list of output directories written
    (empty if everything was already done).  batch_reps: the reps of a barcode session that are still to do go through the
    library in one B = reps call (reconstruct_batch) instead of one call per rep (with register, every rep under its own table); `loaded`: frames already decoded by a
    Prefetcher (what load_corner_reps / load_mono_cal_session / load_rgb_cal_combo would return).  row_bands (the two cal_target
    kinds: one large image per session): all ranks work on this one session (reconstruct(row_bands=True)), rank 0 writes.
    register: reconstruct with shifts estimated from the frames (register_shifts) and write registration.json beside the PNGs.
    keep_u8 (run_sr --u8-frames): the frames this call loads itself stay uint8 on the device; the files written are the same.
    device_png (run_sr --png-on-device): the PNGs' streams are compressed on the device (_save_outputs): the same pixels in every file.
    patchwise (run_sr --patchwise; the two cal_target kinds): "global" or "local", reconstruct's argument, with patch_opts the keywords
    of patchwise.PatchGrid; "local" writes shift_field.json (the grid, the patch centres, estimated / used / score / status) beside the PNGs.
    colour (run_sr --colour; the two rgb_* kinds, not with patchwise or row_bands): all four Bayer planes are reconstructed as one batch
    under the one table (reconstruct_colour; with register the shifts are measured on the red planes, as without it), every file of the
    plain run is written byte for byte, and beside them native_2x_rgb.png, SAA_rgb.png, SAA_IBP_rgb.png and convergence_planes.json (the
    four planes' MSE traces).  `loaded` must then come from load_session(..., colour=True)."""
    kind = kind or detect_kind(session_dir)
    if kind not in IBP_ITERATIONS:
        raise ValueError("kind must be one of " + ", ".join(IBP_ITERATIONS))
    _check_colour(colour, kind, patchwise, row_bands)
    if patchwise is not None and (kind not in ("mono_cal_target", "rgb_cal_target") or row_bands):
        raise ValueError("patchwise is for the one-image-per-session kinds, and not together with row_bands")
    n_iter = IBP_ITERATIONS[kind] if n_iter is None else n_iter
    name = os.path.basename(os.path.normpath(session_dir))
    say = print if verbose else (lambda *a, **k: None)
    written = []
    if kind in ("mono_cal_target", "rgb_cal_target"):
        out_dir = os.path.join(output_base, name)
        if os.path.exists(os.path.join(out_dir, "done.flag")):
            say(f"  [skip] {name} - already done")
            return written
        if kind == "mono_cal_target":
            frames, shifts = loaded or load_mono_cal_session(session_dir, keep_u8=keep_u8)
            lr_name, extra = "LR_mean.png", None
        else:
            frames, shifts = loaded or load_rgb_cal_combo(session_dir, keep_u8=keep_u8, planes="all" if colour else "red")
            lr_name = "LR_red_mean.png"
            extra = {"shifts.json": {"shifts_lr_yx": [list(s) for s in shifts], "corner_labels": CORNER_ORDER}}
        if register:
            shifts, reg = register_shifts([[f[0] for f in frames] if colour else frames], shifts)[0]
            extra = dict(extra or {}, **{"registration.json": reg})
        rgb = None
        if colour:
            rgb, plane_images, traces = reconstruct_colour(frames, shifts, psf_kernel, n_iter)
            images, errors = plane_images[0], traces[0]
            extra = dict(extra, **{"convergence_planes.json": {"ibp_mse": traces}})
        else:
            images, errors = reconstruct(frames, shifts, psf_kernel, n_iter, row_bands=row_bands, patchwise=patchwise, patch_opts=patch_opts)
        if "shift_field" in images:
            extra = dict(extra or {}, **{"shift_field.json": images.pop("shift_field")})
        if images["SAA_IBP"] is None:  # row-band mode, not rank 0: the assembled image lives on rank 0
            return written
        _save_outputs(out_dir, images, errors, lr_name, extra, device_png=device_png, rgb=rgb)
        if on_images:  # (the device tensors the PNGs were quantised from: metrics without reading the files back)
            on_images(out_dir, images)
        if flush:
            flush_writes()
        say(f"  Output: {out_dir}")
        written.append(out_dir)
        return written
    red = kind == "rgb_barcodes"
    all_reps, shifts = loaded or load_corner_reps(session_dir, "all" if colour else red, keep_u8=keep_u8)
    todo = []
    for rep_idx, frames in enumerate(all_reps):
        out_dir = os.path.join(output_base, name, f"rep{rep_idx}")
        if os.path.exists(os.path.join(out_dir, "done.flag")):
            say(f"  [skip] rep {rep_idx} - already done")
            continue
        todo.append((out_dir, frames))
    if not todo:
        return written
    extras, rgbs = [None] * len(todo), [None] * len(todo)
    if colour:  # the reps x 4 planes as one batch; registration, as below, on the red planes
        tables, extras = shifts, [{} for _ in todo]
        if register:
            regs = register_shifts([[f[0] for f in fr] for _, fr in todo], shifts)
            tables, extras = [used for used, _ in regs], [{"registration.json": reg} for _, reg in regs]
        if batch_reps:
            colour_results = reconstruct_colour_batch([fr for _, fr in todo], tables, psf_kernel, n_iter)
        else:
            colour_results = [reconstruct_colour(fr, tables[k] if register else tables, psf_kernel, n_iter) for k, (_, fr) in enumerate(todo)]
        results, rgbs = [(planes[0], traces[0]) for _, planes, traces in colour_results], [rgb for rgb, _, _ in colour_results]
        for extra, (_, _, traces) in zip(extras, colour_results):
            extra["convergence_planes.json"] = {"ibp_mse": traces}
    elif register:  # one registration item per rep (one batched call); each rep then reconstructs with its own shifts
        regs = register_shifts([fr for _, fr in todo], shifts)
        if batch_reps:  # ... in one library call per stage, each with its own table
            results = reconstruct_batch([fr for _, fr in todo], [used for used, _ in regs], psf_kernel, n_iter, lazy_errors=True)
        else:
            results = [reconstruct(fr, used, psf_kernel, n_iter) for (_, fr), (used, _) in zip(todo, regs)]
        extras = [{"registration.json": reg} for _, reg in regs]
    elif batch_reps:
        results = reconstruct_batch([fr for _, fr in todo], shifts, psf_kernel, n_iter, lazy_errors=True)
    else:
        results = [reconstruct(fr, shifts, psf_kernel, n_iter) for _, fr in todo]
    for (out_dir, _), (images, errors), extra, rgb in zip(todo, results, extras, rgbs):
        _save_outputs(out_dir, images, errors, "LR_red_mean.png" if red else "LR_mean.png", extra, device_png=device_png, rgb=rgb)
        say(f"    Output: {out_dir}")
        written.append(out_dir)
    if flush:
        flush_writes()
    return written


def _check_colour(colour, kind, patchwise, row_bands):
    if colour and kind not in ("rgb_cal_target", "rgb_barcodes"):
        raise ValueError("colour is for the two rgb_* kinds (raw RGGB frames)")
    if colour and (patchwise is not None or row_bands):
        raise ValueError("colour goes with neither patchwise nor row_bands")


def load_session(session_dir, kind, keep_u8=False, colour=False):
    """The host + upload half of process_session (what a Prefetcher runs ahead): decoded frames on the device.  keep_u8: as uint8 where
    the kind's frames are the camera's samples (rgb_cal_target averages its reps: float64 frames either way, formed from the bytes by
    mean_u8 with keep_u8).  colour (the two rgb_* kinds): every frame is the [4, h, w] stack of its Bayer planes."""
    if kind == "mono_cal_target":
        return load_mono_cal_session(session_dir, keep_u8=keep_u8)
    if kind == "rgb_cal_target":
        return load_rgb_cal_combo(session_dir, keep_u8=keep_u8, planes="all" if colour else "red")
    return load_corner_reps(session_dir, "all" if colour and kind == "rgb_barcodes" else kind == "rgb_barcodes", keep_u8=keep_u8)


def process_sessions(sessions, psf_kernel, output_base, kind, n_iter=None, verbose=True, rank=0, world=1, on_written=None, row_bands=False,
                     on_images=None, register=False, keep_u8=False, device_png=False, patchwise=None, patch_opts=None, colour=False):
    """The reference's outer loop (mono_cal_target/run_sr.py:358-360, mono_barcodes/run_sr.py:301) over the sessions this
    rank owns (session i -> rank i mod world, parallel.map_sharded: independent items, no data-path collective), with the PNG
    decode and upload of session k + 1 overlapped with the device work of session k.  -> output directories written: by every
    rank's sessions, in session order, on rank 0 (one gather of the directory names when the job ends); [] on the other ranks of a
    process group (a caller playing one rank of several WITHOUT a group gets its own share's directories).  With a process group,
    `rank` / `world` must be the group's (ValueError otherwise: ownership and the gather would disagree).
    row_bands: the other way to use several GPUs -- every rank walks ALL sessions and each image is split into row bands."""
    from . import parallel
    if row_bands and kind not in ("mono_cal_target", "rgb_cal_target"):
        raise ValueError("row_bands is for the one-image-per-session kinds (the barcode kinds batch their reps instead)")
    if patchwise is not None and (kind not in ("mono_cal_target", "rgb_cal_target") or row_bands):
        raise ValueError("patchwise is for the one-image-per-session kinds, and not together with row_bands")
    _check_colour(colour, kind, patchwise, row_bands)
    owned = list(range(len(sessions))) if row_bands else parallel.shard_indices(len(sessions), rank, world)
    say = print if verbose else (lambda *a, **k: None)

    def load(i):
        name = os.path.basename(os.path.normpath(sessions[i]))
        if kind in ("mono_cal_target", "rgb_cal_target") and os.path.exists(os.path.join(output_base, name, "done.flag")):
            return None  # process_session will skip it: do not decode
        return load_session(sessions[i], kind, keep_u8=keep_u8, colour=colour)

    feed = iter(Prefetcher(owned, load))
    count = [0]

    def one(i):
        j, loaded = next(feed)  # the prefetcher walks the owned sessions in the same order map_sharded does
        assert j == i
        count[0] += 1
        say(f"\n[rank {rank}: {count[0]}/{len(owned)}] {os.path.basename(sessions[i])}")
        out = process_session(sessions[i], psf_kernel, output_base, kind=kind, n_iter=n_iter, verbose=verbose, loaded=loaded,
                              flush=on_written is not None, row_bands=row_bands, on_images=on_images, register=register, device_png=device_png,
                              patchwise=patchwise, patch_opts=patch_opts, colour=colour)
        if on_written:
            for d in out:
                on_written(d)
        return out

    try:
        import torch.distributed as dist
        if row_bands or world == 1 or not (dist.is_available() and dist.is_initialized()):
            per_session = [one(i) for i in owned]  # (a caller playing one rank of several without a process group gets its own share)
        else:
            if dist.get_rank() != rank or dist.get_world_size() != world:
                raise ValueError(f"rank / world ({rank} / {world}) are not the process group's ({dist.get_rank()} / {dist.get_world_size()})")
            per_session = parallel.map_sharded(one, len(sessions))
    finally:
        feed.close()  # shuts the decode thread down, also when a session raised
        flush_writes()  # the PNG encodes of session k ran beside the device work of session k + 1
    if per_session is None:  # not rank 0 of a sharded job
        return []
    return [d for out in per_session for d in out]


def write_metrics_device(out_dir, images, factor=UPSAMPLE_FACTOR):
    """metrics.json for one mono_cal_target output directory from the DEVICE tensors of the reconstruction (process_session's
    on_images hook): the notebook's summary (analysis.ipynb cells 3-10) on the values the PNGs hold -- clamped and truncated to 0..255,
    run_sr.py:303 -- with every pass over a frame or an ROI in libsrx (sr_mi355x/metrics_device.py), plus the full-frame PSNR figures
    of SAA+IBP against the two baselines (one fused reduction over two 12.6 MP device images each; the affine-fit form is the vendor
    GUI's comparison, XPR_Software.py:735-745, 1215-1256)."""
    from . import metrics_device as md
    q = {n: api.u8_to_float(api.quantize_u8(images[n]), precision="f32") for n in ("native_2x", "SAA", "SAA_IBP")}  # 0..255 integers, on the device
    rep = md.cal_target_report(q, factor=factor)
    rep["psnr_db"] = {f"SAA_IBP_vs_{n}": {"plain": md.psnr(q[n], q["SAA_IBP"]), "affine_fit": float(md.psnr_affine(q[n], q["SAA_IBP"]))}
                      for n in ("native_2x", "SAA")}
    with open(os.path.join(out_dir, "metrics.json"), "w") as fp:
        json.dump(rep, fp, indent=2)
    return rep


def queue_metrics_device(out_dir, images, factor=UPSAMPLE_FACTOR):
    """write_metrics_device's metrics.json without a wait on the calling thread (process_session's on_images hook; run_sr
    --metrics-on-device).  Everything is queued: the three ROIs go from the quantised BYTES through one srx_edge_sfr_u8 call
    (metrics_device.edge_sfr: threshold, line fits, ESF, MTF50 / MTF10 on the device), the four PSNR reductions are two B = 2
    pair-moment calls (borders 0 and 10), the three bar profiles one local-contrast call; the results are copied into pinned buffers
    behind one event, and a job of the writer pool waits for it, finishes the few host operations (cycles/mm, the PSNR formulas, the
    mean) and writes the file.  flush_writes() covers the job.  Same values as write_metrics_device within rounding.
    Two things follow from the queue.  An item whose status is not 0 (too few edge pixels, ...) raises RuntimeError inside the job, so
    the error surfaces at flush_writes(), not at this call.  And the job is separate from _save_outputs' PNG jobs, whose last one
    writes done.flag: as with write_metrics_device, a run interrupted between the two leaves a directory that is marked done and has no
    metrics.json, and a rerun skips it (session.write_metrics(out_dir) computes the report from the PNGs of such a directory)."""
    import torch
    from . import metrics_device as md
    names = ("native_2x", "SAA", "SAA_IBP")
    q = [api.quantize_u8(images[n]) for n in names]
    for n, t in zip(names, q):
        if tuple(t.shape) != (1536 * factor, 2048 * factor):
            raise ValueError(f"{n}: the notebook's ROIs are defined on the {1536 * factor} x {2048 * factor} cal-target frame")
    sfr = md.edge_sfr(torch.stack([md._roi2(t, factor) for t in q])).start_copy()
    qf = api.u8_to_float(torch.stack(q + [q[2]]), precision="f32")  # native_2x, SAA | SAA_IBP twice: ref = qf[:2], test = qf[2:]
    moments = torch.stack([md.pair_moments_device(qf[:2], qf[2:], border=0), md.pair_moments_device(qf[:2], qf[2:], border=10)])
    contrast = md.local_contrast_device(torch.stack([md._profile1(t, factor) for t in q]), window=16)

    def to_host(t):
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        return h

    mom_host, ct_host = to_host(moments), to_host(contrast)
    ready = torch.cuda.Event()
    ready.record()

    def job():
        ready.synchronize()
        rep = md.report_from_sfr(names, sfr.result(), ct_host.numpy(), factor)
        mom = mom_host.numpy()
        rep["psnr_db"] = {f"SAA_IBP_vs_{n}": {"plain": md.psnr_from_moments(mom[0, k]), "affine_fit": float(md.psnr_affine_from_moments(mom[1, k]))}
                          for k, n in enumerate(names[:2])}
        with open(os.path.join(out_dir, "metrics.json"), "w") as fp:
            json.dump(rep, fp, indent=2)
        return rep

    _pending.append(_writer_pool().submit(job))


def write_metrics(out_dir, factor=UPSAMPLE_FACTOR):
    """metrics.json for one mono_cal_target output directory: the reference's notebook summary (analysis.ipynb cells
    3-10) computed from the uint8 PNGs just written, as the notebook does."""
    import numpy as np
    from PIL import Image
    from . import metrics
    imgs = {n: np.array(Image.open(os.path.join(out_dir, n + ".png")), dtype=np.float64) for n in ("native_2x", "SAA", "SAA_IBP")}
    rep = metrics.cal_target_report(imgs, factor=factor)
    with open(os.path.join(out_dir, "metrics.json"), "w") as fp:
        json.dump(rep, fp, indent=2)
    return rep


def discover_sessions(data_dir, kind):
    """main()'s session discovery (mono_cal_target/run_sr.py:338-343 and the corner-layout variants)."""
    out = []
    for d in sorted(os.listdir(data_dir)):
        full = os.path.join(data_dir, d)
        if not os.path.isdir(full):
            continue
        names = os.listdir(full)
        if kind == "mono_cal_target":
            ok = "center.png" in names
        elif kind == "rgb_cal_target":
            ok = "metadata.json" in names
        else:
            ok = any(re.match(r"corner\d+_rep\d+\.png", n) for n in names)
        if ok:
            out.append(full)
    if not out:
        raise FileNotFoundError(f"No session folders found in {data_dir}")
    return out


# ---------------------------------------------------------------------------------------------------------
# measured PSF (load_measured_psf, mono_cal_target/run_sr.py:114-152): host side, once per run, tiny
# ---------------------------------------------------------------------------------------------------------
def psf_from_pinhole_images(images, halfwidth=PSF_HALFWIDTH):
    """images: iterable of 2-D arrays (pinhole frames).  The brightest pixel of every frame is brought to the centre of a
    (2 (halfwidth + 6) + 1)^2 window (frames whose window would leave the image are dropped); the windows' mean is cut to its
    central (2 halfwidth + 1)^2, the mean of the four 3 x 3 corner blocks is taken off as background, negatives are clipped and
    the kernel normalised to sum 1 (load_measured_psf, mono_cal_target/run_sr.py:114-152)."""
    reach, side = halfwidth + 6, 2 * halfwidth + 1
    span = np.arange(-reach, reach + 1)
    windows = []
    for frame in images:
        frame = np.asarray(frame, dtype=np.float64)
        peak = np.array(np.unravel_index(np.argmax(frame), frame.shape))
        if np.all(peak >= reach) and np.all(peak + reach < np.array(frame.shape)):
            windows.append(frame[np.ix_(peak[0] + span, peak[1] + span)])
    if not windows:
        raise FileNotFoundError("no usable pinhole image")
    core = np.stack(windows).mean(axis=0)[6:6 + side, 6:6 + side]
    edge = np.r_[0:3, side - 3:side]  # the three outermost rows / columns on either side
    core = np.maximum(core - core[np.ix_(edge, edge)].mean(), 0.0)
    return core / core.sum()


def load_measured_psf(psf_dir):
    """Average the pos4_(0,0).png pinhole frames of every sweep directory (run_sr.py:114-152)."""
    imgs = []
    for sweep in sorted(os.listdir(psf_dir)):
        path = os.path.join(psf_dir, sweep, "pos4_(0,0).png")
        if os.path.isdir(os.path.join(psf_dir, sweep)) and os.path.exists(path):
            a = _png_u8(path)
            imgs.append(a.astype(np.float64))
    if not imgs:
        raise FileNotFoundError(f"No pos4_(0,0).png found under {psf_dir}")
    return psf_from_pinhole_images(imgs)


def load_measured_psf_device(psf_dir):
    """load_measured_psf with everything behind the PNG decode on the device: the same discovery, the files decoded side by side
    (_decode_many), the uint8 frames uploaded as they are and handed to psf_device.estimate_psf (srx_psf_estimate_u8)."""
    from . import psf_device
    paths = []
    for sweep in sorted(os.listdir(psf_dir)):
        path = os.path.join(psf_dir, sweep, "pos4_(0,0).png")
        if os.path.isdir(os.path.join(psf_dir, sweep)) and os.path.exists(path):
            paths.append(path)
    if not paths:
        raise FileNotFoundError(f"No pos4_(0,0).png found under {psf_dir}")
    imgs = _decode_many(paths)
    if api._is_u8(imgs):
        return psf_device.estimate_psf(imgs)
    with _loader_precision():  # colour files: load_gray's channel mean, float64
        return psf_device.estimate_psf([a.astype(np.float64) for a in imgs])
