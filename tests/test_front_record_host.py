"""The Python front-end's path from caller data to the library, recorded without a GPU: which libsrx symbol every public wrapper calls,
with how many arguments, and the dtype, shape and contiguity of every tensor whose pointer it hands over -- for every kind of input the
coercion rules tell apart (numpy uint8 / float32 / float64 / int16, lists of arrays and of tensors, torch uint8 / float32 / float64 / int16,
non-contiguous views, [H, W] where the batch is optional), and the exception type of every input a wrapper rejects.

The library is a fake whose every symbol records itself and returns 0 (b"" where the real one returns a string), api._device is the CPU,
api._stream is None and api._p records the tensor instead of taking its address: the wrappers then run on the CPU up to and including the
library call.  Nothing is computed, so the outputs hold whatever torch.empty left and only their kind is recorded.

EXPECTED holds literals.  One line per library call, "symbol(argument count) <- the tensors passed to it, in order"; a last line for what
came back ("-> ...") or was raised ("raises ..."); equal neighbours are written once, as "n x ...".  The input kinds of one case that give
the same record share an entry.  The literals were taken by running these cases on the front-end as it stood before the coercion rules
were gathered in api.py, and the file uses public names and the front-end's long-standing private seams only (api._device, _p, _stream,
_lib.load; session._to_dev_f, _to_dev_frames, _frame_mean), so that it passes unchanged on either side of that change."""
import json
import warnings

import numpy as np
import pytest
import torch

from sr_mi355x import _lib, api, metrics_device, patchwise, psf_device, register, session, synth

_DT = {torch.uint8: "u8", torch.float32: "f32", torch.float64: "f64", torch.int64: "i64", torch.int32: "i32", torch.int16: "i16"}


def describe(v):
    if isinstance(v, torch.Tensor):
        return f"{_DT.get(v.dtype, v.dtype)}{list(v.shape)}".replace(" ", "") + ("" if v.is_contiguous() else "!strided")
    if isinstance(v, np.ndarray):
        return f"np.{v.dtype}{list(v.shape)}".replace(" ", "")
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {describe(e)}" for k, e in v.items()) + "}"
    if isinstance(v, (tuple, list)):
        return "(" + ", ".join(_runs([describe(e) for e in v])) + ")"
    return type(v).__name__


def _runs(items):
    """equal neighbours as one "n x item" """
    out = []
    for it in items:
        if out and out[-1][0] == it:
            out[-1][1] += 1
        else:
            out.append([it, 1])
    return [it if n == 1 else f"{n} x {it}" for it, n in out]


class Recorder:
    """the fake library and the fake api._p; `lines` is the record of one call of a wrapper"""

    def __init__(self):
        self.lines, self.pending = [], []

    def __getattr__(self, symbol):
        def fn(*args):
            self.lines.append(f"{symbol}({len(args)})" + (" <- " + " ".join(self.pending) if self.pending else ""))
            self.pending = []
            return b"" if "_path" in symbol or symbol == "srx_strerror" else 0
        return fn

    def p(self, t):
        self.pending.append(describe(t))

    def take(self, fn, *args):
        self.lines, self.pending = [], []
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            try:
                self.lines.append("-> " + describe(fn(*args)))
            except Exception as e:  # noqa: BLE001  (the type is what is recorded)
                self.lines.append("raises " + type(e).__name__)
        return _runs(self.lines)


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    grid()  # (the real library's srx_patches_count, before the fake takes its place)
    monkeypatch.setattr(_lib, "load", lambda: r)
    monkeypatch.setattr(api, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(api, "_stream", lambda: None)
    monkeypatch.setattr(api, "_p", r.p)
    return r


_grid = []


def grid():
    """2 x 2 patches of 40 x 40 (the smallest registration admits with its default border and search) on a 48 x 48 frame"""
    if not _grid:
        _grid.append(patchwise.PatchGrid(48, 48, 2, patch_lr=40, overlap_lr=16, margin_hr=8))
    return _grid[0]


def kinds(shape, lists=False):
    """every kind of input the rules tell apart, all zeros, of one shape; lists: also as sequences of its frames"""
    z = np.zeros(shape)
    wide = np.zeros(tuple(shape[:-1]) + (2 * shape[-1],))
    k = {"np_u8": z.astype(np.uint8), "np_f32": z.astype(np.float32), "np_f64": z, "np_i16": z.astype(np.int16),
         "t_u8": torch.zeros(shape, dtype=torch.uint8), "t_f32": torch.zeros(shape, dtype=torch.float32),
         "t_f64": torch.zeros(shape, dtype=torch.float64), "t_i16": torch.zeros(shape, dtype=torch.int16),
         "np_u8_strided": wide.astype(np.uint8)[..., ::2], "np_f32_strided": wide.astype(np.float32)[..., ::2],
         "t_u8_strided": torch.from_numpy(wide.astype(np.uint8))[..., ::2], "t_f32_strided": torch.from_numpy(wide.astype(np.float32))[..., ::2]}
    if lists:
        k.update({"list_np_u8": list(k["np_u8"]), "list_np_f32": list(k["np_f32"]), "list_np_f64": list(z), "list_t_u8": list(k["t_u8"]),
                  "list_t_f32": list(k["t_f32"]), "list_t_f64": list(k["t_f64"]), "list_np_mixed": [k["np_u8"][0]] + list(z[1:]),
                  "list_t_mixed": [k["t_u8"][0]] + list(k["t_f64"][1:]), "tuple_np_u8": tuple(k["np_u8"]), "nested_lists": z.tolist()})
    return k


PSF = synth.gaussian_psf()
T4 = synth.NOMINAL_4
T4_ITEMS = np.asarray(T4, dtype=np.float64)[None]   # [1, 4, 2]: one table per item
T3 = [(0.0, 0.0), (0.5, -0.5), (-0.5, 0.5)]
HR0 = np.zeros((1, 16, 16))
LR_F32 = torch.zeros((1, 4, 8, 8), dtype=torch.float32)
LR_U8 = torch.zeros((1, 4, 8, 8), dtype=torch.uint8)


def _psf(frames, **kw):
    """estimate_psf up to and including the library call: whether a frame counts as used is read from an output the fake never writes"""
    try:
        psf_device.estimate_psf(frames, **kw)
    except FileNotFoundError:
        pass


def _plan(x):
    plan = api.IbpPlan(x, T4, PSF, HR0)
    return plan.lr, plan.B, plan.N, plan.h, plan.w, plan.H, plan.W


# case id -> (the shape of the input that varies, whether it is also given as sequences of frames, the call)
CASES = {
    "saa_batched": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_batched(x, T4, 2)),
    "saa_batched.items": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_batched(x, T4_ITEMS, 2)),
    "saa_batched.f64": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_batched(x, T4, 2, precision="f64")),
    "saa_batched.rank3": ((4, 8, 8), False, lambda x: api.shift_and_add_batched(x, T4, 2)),
    "saa_u8_batched": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_u8_batched(x, T4, 2)),
    "saa_u8_batched.items": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_u8_batched(x, T4_ITEMS, 2)),
    "saa_u8_batched.f64": ((1, 4, 8, 8), False, lambda x: api.shift_and_add_u8_batched(x, T4, 2, precision="f64")),
    "saa_u8_batched.rank3": ((4, 8, 8), False, lambda x: api.shift_and_add_u8_batched(x, T4, 2)),
    "ibp_batched": ((1, 4, 8, 8), False, lambda x: api.ibp_batched(x, T4, PSF, HR0, 2, 1)),
    "ibp_batched.items": ((1, 4, 8, 8), False, lambda x: api.ibp_batched(x, T4_ITEMS, PSF, HR0, 2, 1)),
    "ibp_batched.f64": ((1, 4, 8, 8), False, lambda x: api.ibp_batched(x, T4, PSF, HR0, 2, 1, precision="f64")),
    "ibp_batched.bound_no_errors": ((1, 4, 8, 8), False, lambda x: api.ibp_batched(x, T4, PSF, HR0, 2, 1, want_errors=False, exact_workspace=False)),
    "ibp_batched.hr_init": ((1, 16, 16), False, lambda x: api.ibp_batched(LR_F32, T4, PSF, x, 2, 1)),
    "ibp_batched.hr_init_batch_of_2": ((2, 16, 16), False, lambda x: api.ibp_batched(LR_F32, T4, PSF, x, 2, 1)),
    "ibp_batched.out_on_the_host": ((1, 16, 16), False, lambda x: api.ibp_batched(LR_F32, T4, PSF, HR0, 2, 1, out=x)),
    "ibp_u8_batched": ((1, 4, 8, 8), False, lambda x: api.ibp_u8_batched(x, T4, PSF, HR0, 2, 1)),
    "ibp_u8_batched.items": ((1, 4, 8, 8), False, lambda x: api.ibp_u8_batched(x, T4_ITEMS, PSF, HR0, 2, 1)),
    "ibp_u8_batched.f64": ((1, 4, 8, 8), False, lambda x: api.ibp_u8_batched(x, T4, PSF, HR0, 2, 1, precision="f64")),
    "ibp_u8_batched.bound_no_errors": ((1, 4, 8, 8), False, lambda x: api.ibp_u8_batched(x, T4, PSF, HR0, 2, 1, want_errors=False, exact_workspace=False)),
    "ibp_u8_batched.hr_init": ((1, 16, 16), False, lambda x: api.ibp_u8_batched(LR_U8, T4, PSF, x, 2, 1)),
    "ibp_u8_batched.hr_init_batch_of_2": ((2, 16, 16), False, lambda x: api.ibp_u8_batched(LR_U8, T4, PSF, x, 2, 1)),
    "ibp_u8_batched.out_on_the_host": ((1, 16, 16), False, lambda x: api.ibp_u8_batched(LR_U8, T4, PSF, HR0, 2, 1, out=x)),
    "IbpPlan": ((1, 4, 8, 8), False, _plan),
    "blur": ((8, 8), False, lambda x: api.blur(x, PSF)),
    "zoom_batched": ((1, 8, 8), False, lambda x: api.zoom_batched(x, 2)),
    "shift_and_add": ((4, 8, 8), True, lambda x: api.shift_and_add(x, T4, 2)),
    "ibp": ((4, 8, 8), True, lambda x: api.ibp(x, T4, PSF, HR0[0], 2, 1, verbose=False)),
    "decimate": ((8, 8), False, lambda x: api.decimate(x, 2)),
    "decimate_u8": ((8, 8), False, lambda x: api.decimate_u8(x, 2)),
    "decimate_u8.batch": ((2, 8, 8), False, lambda x: api.decimate_u8(x, 2, 1, 1)),
    "decimate_u8.rank4": ((1, 2, 8, 8), False, lambda x: api.decimate_u8(x, 2)),
    "mean_frames": ((3, 8, 8), True, api.mean_frames),
    "mean_frames_batched": ((2, 3, 8, 8), False, api.mean_frames_batched),
    "mean_u8": ((1, 3, 8, 8), False, lambda x: api.mean_u8(x, 2)),
    "mean_u8.f64": ((1, 3, 8, 8), False, lambda x: api.mean_u8(x, precision="f64")),
    "mean_u8.rank3": ((3, 8, 8), False, api.mean_u8),
    "quantize_u8": ((8, 8), False, api.quantize_u8),
    "png_deflate": ((8, 8), False, api.png_deflate),
    "png_deflate.batch": ((2, 8, 8), True, api.png_deflate),
    "png_file": ((8, 8), False, api.png_file),
    "png_file.batch": ((2, 8, 8), True, api.png_file),
    "png_file.rank4": ((1, 2, 8, 8), False, api.png_file),
    "crc32": ((16,), False, api.crc32),
    "crc32.batch": ((2, 16), False, lambda x: api.crc32(x, np.array([3, 16], dtype=np.int32), seed=7)),
    "crc32.lengths_on_the_device": ((2, 16), False, lambda x: api.crc32(x, torch.tensor([3, 16], dtype=torch.int32))),
    "crc32.lengths_of_another_batch": ((2, 16), False, lambda x: api.crc32(x, [3, 16, 4])),
    "crc32.rank3": ((2, 4, 4), False, api.crc32),
    "crc32.no_bytes": ((2, 0), False, api.crc32),
    "u8_to_float": ((8, 8), False, api.u8_to_float),
    "u8_to_float.f64": ((2, 8, 8), False, lambda x: api.u8_to_float(x, "f64")),
    "interleave4": ((4, 8, 8), True, api.interleave4),
    "interleave4.batch": ((2, 4, 8, 8), False, api.interleave4),
    "interleave4.three_frames": ((3, 8, 8), False, api.interleave4),
    "estimate_shifts": ((3, 40, 40), True, register.estimate_shifts),
    "estimate_shifts.batch_full": ((2, 3, 40, 40), False, lambda x: register.estimate_shifts(x, init=T3, full=True)),
    "estimate_shifts.f64": ((3, 40, 40), False, lambda x: register.estimate_shifts(x, precision="f64")),
    "estimate_shifts.frame_too_small": ((3, 39, 40), True, register.estimate_shifts),
    "estimate_psf": ((2, 40, 40), True, _psf),
    "estimate_psf.f64": ((2, 40, 40), False, lambda x: _psf(x, precision="f64", halfwidth=2)),
    "estimate_psf.one_frame_is_no_stack": ((40, 40), False, _psf),
    "gather": ((4, 48, 48), False, lambda x: patchwise.gather(x, grid())),
    "gather.batch": ((2, 4, 48, 48), False, lambda x: patchwise.gather(x, grid())),
    "gather.another_frame_size": ((4, 48, 40), False, lambda x: patchwise.gather(x, grid())),
    "blend": ((4, 80, 80), False, lambda x: patchwise.blend(x, grid())),
    "blend.not_the_grid_s_patches": ((3, 80, 80), False, lambda x: patchwise.blend(x, grid())),
    "estimate_shift_field": ((3, 48, 48), True, lambda x: patchwise.estimate_shift_field(x, T3, grid())),
    "pair_moments_device.ref": ((8, 8), False, lambda x: metrics_device.pair_moments_device(x, np.zeros((8, 8)))),
    "pair_moments_device.test": ((8, 8), False, lambda x: metrics_device.pair_moments_device(torch.zeros((8, 8)), x, border=1)),
    "pair_moments_device.test_of_an_array": ((2, 8, 8), False, lambda x: metrics_device.pair_moments_device(np.zeros((2, 8, 8), np.float32), x)),
    "pair_moments_device.shapes_differ": ((8, 9), False, lambda x: metrics_device.pair_moments_device(torch.zeros((8, 8)), x)),
    "ssim.ref": ((16, 16), False, lambda x: metrics_device.ssim(x, np.zeros((16, 16)), full=True)),
    "ssim.test": ((2, 16, 16), False, lambda x: metrics_device.ssim(torch.zeros((2, 16, 16)), x, data_range=255.0)),
    "ssim.rank4": ((1, 1, 16, 16), False, lambda x: metrics_device.ssim(x, x)),
    "ssim_affine": ((16, 16), False, lambda x: metrics_device.ssim_affine(x, x, border=2)),
    "ecc": ((2, 8, 8), False, lambda x: metrics_device.ecc(x, x)),
    "local_contrast": ((16,), False, lambda x: metrics_device.local_contrast(x, 4)),
    "local_contrast.batch": ((2, 16), False, lambda x: metrics_device.local_contrast(x, 4)),
    "local_contrast_device": ((2, 16), False, lambda x: metrics_device.local_contrast_device(x, 4)),
    "radial_average": ((8, 8), False, metrics_device.radial_average),
    "subpixel_centre": ((8, 8), False, metrics_device.subpixel_centre),
    "edge_magnitude": ((8, 8), False, metrics_device.edge_magnitude),
}

U8 = "np_u8 t_u8 np_u8_strided t_u8_strided"
U8_LISTS = U8 + " list_np_u8 list_t_u8 tuple_np_u8"
TENSORS = "t_u8 t_f32 t_f64 t_i16 t_u8_strided t_f32_strided"
TENSOR_LISTS = TENSORS + " list_t_u8 list_t_f32 list_t_f64 list_t_mixed"
F32 = "np_f32 t_f32 np_f32_strided t_f32_strided"
FIELD = "-> {estimated: np.float64[2,2,3,2], used: np.float64[2,2,3,2], score: np.float64[2,2,3], status: np.int32[2,2,3]}"

# case id -> {input kinds, "*" for every kind no other entry of the case names: the record}
EXPECTED = {
    "saa_batched": {
        "*": ["srx_saa_workspace_bytes(6)", "srx_saa_f32(12) <- f32[1,4,8,8] f32[1,16,16]", "-> f32[1,16,16]"],
    },
    "saa_batched.items": {
        "*": ["srx_saa_items_workspace_bytes(6)", "srx_saa_items_f32(12) <- f32[1,4,8,8] f32[1,16,16]", "-> f32[1,16,16]"],
    },
    "saa_batched.f64": {
        "*": ["srx_saa_workspace_bytes(6)", "srx_saa_f64(12) <- f64[1,4,8,8] f64[1,16,16]", "-> f64[1,16,16]"],
    },
    "saa_batched.rank3": {
        "*": ["raises ValueError"],
    },
    "saa_u8_batched": {
        U8: ["srx_saa_u8lr_workspace_bytes(6)", "srx_saa_u8lr_f32(12) <- u8[1,4,8,8] f32[1,16,16]", "-> f32[1,16,16]"],
        "*": ["raises TypeError"],
    },
    "saa_u8_batched.items": {
        U8: ["srx_u8_to_f32(4) <- u8[1,4,8,8] f32[1,4,8,8]",
             "srx_saa_items_workspace_bytes(6)",
             "srx_saa_items_f32(12) <- f32[1,4,8,8] f32[1,16,16]",
             "-> f32[1,16,16]"],
        "*": ["raises TypeError"],
    },
    "saa_u8_batched.f64": {
        U8: ["srx_saa_u8lr_workspace_bytes(6)", "srx_saa_u8lr_f64(12) <- u8[1,4,8,8] f64[1,16,16]", "-> f64[1,16,16]"],
        "*": ["raises TypeError"],
    },
    "saa_u8_batched.rank3": {
        "*": ["raises ValueError"],
    },
    "ibp_batched": {
        "*": ["srx_ibp_workspace_bytes_for(13)", "srx_ibp_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (f32[1,16,16], f64[1,1])"],
    },
    "ibp_batched.items": {
        "*": ["srx_ibp_items_workspace_bytes_for(13)", "srx_ibp_items_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (f32[1,16,16], f64[1,1])"],
    },
    "ibp_batched.f64": {
        "*": ["srx_ibp_workspace_bytes_for(13)", "srx_ibp_f64(21) <- f64[1,4,8,8] f64[1,16,16] f64[1,16,16] f64[1,1]", "-> (f64[1,16,16], f64[1,1])"],
    },
    "ibp_batched.bound_no_errors": {
        "*": ["srx_ibp_workspace_bytes(9)", "srx_ibp_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16]", "-> (f32[1,16,16], NoneType)"],
    },
    "ibp_batched.hr_init": {
        "*": ["srx_ibp_workspace_bytes_for(13)", "srx_ibp_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (f32[1,16,16], f64[1,1])"],
    },
    "ibp_batched.hr_init_batch_of_2": {
        "*": ["raises ValueError"],
    },
    "ibp_batched.out_on_the_host": {
        "*": ["raises ValueError"],
    },
    "ibp_u8_batched": {
        U8: ["srx_ibp_u8lr_workspace_bytes_for(13)", "srx_ibp_u8lr_f32(21) <- u8[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (f32[1,16,16], f64[1,1])"],
        "*": ["raises TypeError"],
    },
    "ibp_u8_batched.items": {
        U8: ["srx_u8_to_f32(4) <- u8[1,4,8,8] f32[1,4,8,8]",
             "srx_ibp_items_workspace_bytes_for(13)",
             "srx_ibp_items_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]",
             "-> (f32[1,16,16], f64[1,1])"],
        "*": ["raises TypeError"],
    },
    "ibp_u8_batched.f64": {
        U8: ["srx_ibp_u8lr_workspace_bytes_for(13)", "srx_ibp_u8lr_f64(21) <- u8[1,4,8,8] f64[1,16,16] f64[1,16,16] f64[1,1]", "-> (f64[1,16,16], f64[1,1])"],
        "*": ["raises TypeError"],
    },
    "ibp_u8_batched.bound_no_errors": {
        U8: ["srx_ibp_u8lr_workspace_bytes(9)", "srx_ibp_u8lr_f32(21) <- u8[1,4,8,8] f32[1,16,16] f32[1,16,16]", "-> (f32[1,16,16], NoneType)"],
        "*": ["raises TypeError"],
    },
    "ibp_u8_batched.hr_init": {
        "*": ["srx_ibp_u8lr_workspace_bytes_for(13)", "srx_ibp_u8lr_f32(21) <- u8[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (f32[1,16,16], f64[1,1])"],
    },
    "ibp_u8_batched.hr_init_batch_of_2": {
        "*": ["raises ValueError"],
    },
    "ibp_u8_batched.out_on_the_host": {
        "*": ["raises ValueError"],
    },
    "IbpPlan": {
        "*": ["srx_ibp_plan_workspace_bytes(9)",
              "srx_ibp_plan_create_f32(21) <- f32[1,4,8,8] f32[1,16,16]",
              "srx_ibp_plan_path(1)",
              "srx_ibp_plan_supports_trace_rows(1)",
              "-> (f32[1,4,8,8], 6 x int)"],
    },
    "blur": {
        "*": ["srx_blur_f32(9) <- f32[1,8,8] f32[1,8,8]", "-> np.float64[8,8]"],
        TENSORS: ["srx_blur_f32(9) <- f32[1,8,8] f32[1,8,8]", "-> f32[8,8]"],
    },
    "zoom_batched": {
        "*": ["srx_zoom_workspace_bytes(5)", "srx_zoom_cubic_f32(9) <- f32[1,8,8] f32[1,16,16]", "-> f32[1,16,16]"],
    },
    "shift_and_add": {
        "*": ["srx_saa_workspace_bytes(6)", "srx_saa_f32(12) <- f32[1,4,8,8] f32[1,16,16]", "-> np.float64[16,16]"],
        TENSOR_LISTS: ["srx_saa_workspace_bytes(6)", "srx_saa_f32(12) <- f32[1,4,8,8] f32[1,16,16]", "-> f32[16,16]"],
    },
    "ibp": {
        "*": ["srx_ibp_workspace_bytes_for(13)", "srx_ibp_f32(21) <- f32[1,4,8,8] f32[1,16,16] f32[1,16,16] f64[1,1]", "-> (np.float64[16,16], (float))"],
    },
    "decimate": {
        "*": ["srx_decimate_f32(9) <- f32[8,8] f32[4,4]", "-> np.float64[4,4]"],
        TENSORS: ["srx_decimate_f32(9) <- f32[8,8] f32[4,4]", "-> f32[4,4]"],
    },
    "decimate_u8": {
        "np_u8 np_u8_strided": ["srx_decimate_u8(9) <- u8[1,8,8] u8[1,4,4]", "-> np.uint8[4,4]"],
        "t_u8 t_u8_strided": ["srx_decimate_u8(9) <- u8[1,8,8] u8[1,4,4]", "-> u8[4,4]"],
        "*": ["raises TypeError"],
    },
    "decimate_u8.batch": {
        "np_u8 np_u8_strided": ["srx_decimate_u8(9) <- u8[2,8,8] u8[2,4,4]", "-> np.uint8[2,4,4]"],
        "t_u8 t_u8_strided": ["srx_decimate_u8(9) <- u8[2,8,8] u8[2,4,4]", "-> u8[2,4,4]"],
        "*": ["raises TypeError"],
    },
    "decimate_u8.rank4": {
        "*": ["raises ValueError"],
    },
    "mean_frames": {
        "*": ["srx_mean_frames_f32(6) <- f32[3,8,8] f32[8,8]", "-> np.float64[8,8]"],
        TENSOR_LISTS: ["srx_mean_frames_f32(6) <- f32[3,8,8] f32[8,8]", "-> f32[8,8]"],
    },
    "mean_frames_batched": {
        "*": ["srx_mean_frames_f32(6) <- f32[2,3,8,8] f32[2,8,8]", "-> np.float64[2,8,8]"],
        TENSORS: ["srx_mean_frames_f32(6) <- f32[2,3,8,8] f32[2,8,8]", "-> f32[2,8,8]"],
    },
    "mean_u8": {
        U8: ["srx_mean_u8(11) <- u8[1,3,8,8] f32[1,4,4]", "-> f32[1,4,4]"],
        "*": ["raises TypeError"],
    },
    "mean_u8.f64": {
        U8: ["srx_mean_u8(11) <- u8[1,3,8,8] f64[1,8,8]", "-> f64[1,8,8]"],
        "*": ["raises TypeError"],
    },
    "mean_u8.rank3": {
        "*": ["raises ValueError"],
    },
    "quantize_u8": {
        "*": ["srx_quantize_u8_f32(4) <- f32[8,8] u8[8,8]", "-> np.uint8[8,8]"],
        TENSORS: ["srx_quantize_u8_f32(4) <- f32[8,8] u8[8,8]", "-> u8[8,8]"],
    },
    "png_deflate": {
        U8: ["srx_png_stream_bound(2)", "srx_png_scratch_bytes(3)", "srx_png_deflate_u8(9) <- u8[1,8,8] u8[1,0] i64[1]", "-> (u8[1,0], i64[1])"],
        "*": ["srx_png_stream_bound(2)", "srx_png_scratch_bytes(3)", "srx_png_deflate_f32(9) <- f32[1,8,8] u8[1,0] i64[1]", "-> (u8[1,0], i64[1])"],
    },
    "png_deflate.batch": {
        U8_LISTS: ["srx_png_stream_bound(2)", "srx_png_scratch_bytes(3)", "srx_png_deflate_u8(9) <- u8[2,8,8] u8[2,0] i64[2]", "-> (u8[2,0], i64[2])"],
        "*": ["srx_png_stream_bound(2)", "srx_png_scratch_bytes(3)", "srx_png_deflate_f32(9) <- f32[2,8,8] u8[2,0] i64[2]", "-> (u8[2,0], i64[2])"],
    },
    "png_file": {
        U8: ["srx_png_file_bound(2)", "srx_png_file_scratch_bytes(3)", "srx_png_file_u8(9) <- u8[1,8,8] u8[1,0] i64[1]", "-> (u8[1,0], i64[1])"],
        "*": ["srx_png_file_bound(2)", "srx_png_file_scratch_bytes(3)", "srx_png_file_f32(9) <- f32[1,8,8] u8[1,0] i64[1]", "-> (u8[1,0], i64[1])"],
    },
    "png_file.batch": {
        U8_LISTS: ["srx_png_file_bound(2)", "srx_png_file_scratch_bytes(3)", "srx_png_file_u8(9) <- u8[2,8,8] u8[2,0] i64[2]", "-> (u8[2,0], i64[2])"],
        "*": ["srx_png_file_bound(2)", "srx_png_file_scratch_bytes(3)", "srx_png_file_f32(9) <- f32[2,8,8] u8[2,0] i64[2]", "-> (u8[2,0], i64[2])"],
    },
    "png_file.rank4": {
        "*": ["raises ValueError"],
    },
    "crc32": {
        U8: ["srx_crc32_scratch_bytes(2)", "srx_crc32(10) <- u8[1,16] i32[1]", "-> i64[1]"],
        "*": ["raises ValueError"],
    },
    "crc32.batch": {
        U8: ["srx_crc32_scratch_bytes(2)", "srx_crc32(10) <- u8[2,16] i64[2] i32[2]", "-> i64[2]"],
        "*": ["raises ValueError"],
    },
    "crc32.lengths_on_the_device": {
        U8: ["srx_crc32_scratch_bytes(2)", "srx_crc32(10) <- u8[2,16] i64[2] i32[2]", "-> i64[2]"],
        "*": ["raises ValueError"],
    },
    "crc32.lengths_of_another_batch": {
        "*": ["raises ValueError"],
    },
    "crc32.rank3": {
        "*": ["raises ValueError"],
    },
    "crc32.no_bytes": {
        U8: ["-> i64[2]"],
        "*": ["raises ValueError"],
    },
    "u8_to_float": {
        "*": ["srx_u8_to_f32(4) <- u8[8,8] f32[8,8]", "-> f32[8,8]"],
    },
    "u8_to_float.f64": {
        "*": ["srx_u8_to_f64(4) <- u8[2,8,8] f64[2,8,8]", "-> f64[2,8,8]"],
    },
    "interleave4": {
        "*": ["srx_interleave4_u8(6) <- u8[1,4,8,8] u8[1,16,16]", "-> np.uint8[16,16]"],
        TENSORS: ["srx_interleave4_u8(6) <- u8[1,4,8,8] u8[1,16,16]", "-> u8[16,16]"],
    },
    "interleave4.batch": {
        "*": ["srx_interleave4_u8(6) <- u8[2,4,8,8] u8[2,16,16]", "-> np.uint8[2,16,16]"],
        TENSORS: ["srx_interleave4_u8(6) <- u8[2,4,8,8] u8[2,16,16]", "-> u8[2,16,16]"],
    },
    "interleave4.three_frames": {
        "*": ["raises ValueError"],
    },
    "estimate_shifts": {
        U8_LISTS: ["srx_register_workspace_bytes(6)", "srx_register_u8_f32(17) <- u8[1,3,40,40] f64[1,3,2] f64[1,3] i32[1,3]", "-> np.float64[3,2]"],
        "*": ["srx_register_workspace_bytes(6)", "srx_register_f32(17) <- f32[1,3,40,40] f64[1,3,2] f64[1,3] i32[1,3]", "-> np.float64[3,2]"],
    },
    "estimate_shifts.batch_full": {
        U8: ["srx_register_workspace_bytes(6)",
             "srx_register_u8_f32(17) <- u8[2,3,40,40] f64[2,3,2] f64[2,3] i32[2,3]",
             "-> (np.float64[2,3,2], np.float64[2,3], np.int32[2,3])"],
        "*": ["srx_register_workspace_bytes(6)",
              "srx_register_f32(17) <- f32[2,3,40,40] f64[2,3,2] f64[2,3] i32[2,3]",
              "-> (np.float64[2,3,2], np.float64[2,3], np.int32[2,3])"],
    },
    "estimate_shifts.f64": {
        U8: ["srx_register_workspace_bytes(6)", "srx_register_u8_f64(17) <- u8[1,3,40,40] f64[1,3,2] f64[1,3] i32[1,3]", "-> np.float64[3,2]"],
        "*": ["srx_register_workspace_bytes(6)", "srx_register_f64(17) <- f64[1,3,40,40] f64[1,3,2] f64[1,3] i32[1,3]", "-> np.float64[3,2]"],
    },
    "estimate_shifts.frame_too_small": {
        "*": ["raises ValueError"],
    },
    "estimate_psf": {
        U8_LISTS: ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_u8(10) <- u8[2,40,40] f64[7,7] i32[2,3]", "-> NoneType"],
        "*": ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_f32(10) <- f32[2,40,40] f64[7,7] i32[2,3]", "-> NoneType"],
    },
    "estimate_psf.f64": {
        U8: ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_u8(10) <- u8[2,40,40] f64[5,5] i32[2,3]", "-> NoneType"],
        "*": ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_f64(10) <- f64[2,40,40] f64[5,5] i32[2,3]", "-> NoneType"],
    },
    "estimate_psf.one_frame_is_no_stack": {
        "*": ["raises ValueError"],
    },
    "gather": {
        U8: ["srx_patches_gather_u8(11) <- u8[1,4,48,48] u8[4,4,40,40]", "-> u8[4,4,40,40]"],
        F32: ["srx_patches_gather_f32(11) <- f32[1,4,48,48] f32[4,4,40,40]", "-> f32[4,4,40,40]"],
        "np_f64 np_i16 t_f64": ["srx_patches_gather_f64(11) <- f64[1,4,48,48] f64[4,4,40,40]", "-> f64[4,4,40,40]"],
        "t_i16": ["raises TypeError"],
    },
    "gather.batch": {
        U8: ["srx_patches_gather_u8(11) <- u8[2,4,48,48] u8[8,4,40,40]", "-> u8[8,4,40,40]"],
        F32: ["srx_patches_gather_f32(11) <- f32[2,4,48,48] f32[8,4,40,40]", "-> f32[8,4,40,40]"],
        "np_f64 np_i16 t_f64": ["srx_patches_gather_f64(11) <- f64[2,4,48,48] f64[8,4,40,40]", "-> f64[8,4,40,40]"],
        "t_i16": ["raises TypeError"],
    },
    "gather.another_frame_size": {
        "*": ["raises ValueError"],
        "t_i16": ["raises TypeError"],
    },
    "blend": {
        U8 + " t_i16": ["raises TypeError"],
        F32: ["srx_patches_blend_f32(11) <- f32[4,80,80] f32[1,96,96]", "-> f32[1,96,96]"],
        "np_f64 np_i16 t_f64": ["srx_patches_blend_f64(11) <- f64[4,80,80] f64[1,96,96]", "-> f64[1,96,96]"],
    },
    "blend.not_the_grid_s_patches": {
        U8 + " t_i16": ["raises TypeError"],
        "*": ["raises ValueError"],
    },
    "estimate_shift_field": {
        U8_LISTS: ["srx_patches_gather_u8(11) <- u8[1,3,48,48] u8[4,3,40,40]",
                   "srx_register_workspace_bytes(6)",
                   "srx_register_u8_f32(17) <- u8[4,3,40,40] f64[4,3,2] f64[4,3] i32[4,3]",
                   FIELD],
        F32 + " list_np_f32 list_t_f32": ["srx_patches_gather_f32(11) <- f32[1,3,48,48] f32[4,3,40,40]",
                                          "srx_register_workspace_bytes(6)",
                                          "srx_register_f32(17) <- f32[4,3,40,40] f64[4,3,2] f64[4,3] i32[4,3]",
                                          FIELD],
        "*": ["srx_patches_gather_f64(11) <- f64[1,3,48,48] f64[4,3,40,40]",
              "srx_register_workspace_bytes(6)",
              "srx_register_f32(17) <- f32[4,3,40,40] f64[4,3,2] f64[4,3] i32[4,3]",
              FIELD],
        "t_i16": ["raises TypeError"],
    },
    "pair_moments_device.ref": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f64(10) <- f64[1,8,8] f64[1,8,8] f64[1,7]", "-> f64[1,7]"],
        "t_f32 t_f32_strided": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f32(10) <- f32[1,8,8] f32[1,8,8] f64[1,7]", "-> f64[1,7]"],
    },
    "pair_moments_device.test": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f32(10) <- f32[1,8,8] f32[1,8,8] f64[1,7]", "-> f64[1,7]"],
    },
    "pair_moments_device.test_of_an_array": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f64(10) <- f64[2,8,8] f64[2,8,8] f64[2,7]", "-> f64[2,7]"],
    },
    "pair_moments_device.shapes_differ": {
        "*": ["raises ValueError"],
    },
    "ssim.ref": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_ssim_f64(18) <- f64[1,16,16] f64[1,16,16] f64[1] f64[1,16,16]", "-> (float, f64[16,16])"],
        F32 + " np_f64 t_f64": ["raises ValueError"],   # (a float image has no default data_range)
    },
    "ssim.test": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_ssim_f32(18) <- f32[2,16,16] f32[2,16,16] f64[2]", "-> (2 x float)"],
    },
    "ssim.rank4": {
        "*": ["raises ValueError"],
    },
    "ssim_affine": {
        "*": ["srx_metrics_workspace_bytes(4)",
              "srx_pair_moments_f64(10) <- f64[1,16,16] f64[1,16,16] f64[1,7]",
              "srx_metrics_workspace_bytes(4)",
              "srx_ssim_f64(18) <- f64[1,16,16] f64[1,16,16] f64[1,3] f64[1]",
              "-> float"],
        "t_f32 t_f32_strided": ["srx_metrics_workspace_bytes(4)",
                                "srx_pair_moments_f32(10) <- f32[1,16,16] f32[1,16,16] f64[1,7]",
                                "srx_metrics_workspace_bytes(4)",
                                "srx_ssim_f32(18) <- f32[1,16,16] f32[1,16,16] f64[1,3] f64[1]",
                                "-> float"],
    },
    "ecc": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f64(10) <- f64[2,8,8] f64[2,8,8] f64[2,7]", "-> (2 x float)"],
        "t_f32 t_f32_strided": ["srx_metrics_workspace_bytes(4)", "srx_pair_moments_f32(10) <- f32[2,8,8] f32[2,8,8] f64[2,7]", "-> (2 x float)"],
    },
    "local_contrast": {
        "*": ["srx_local_contrast_f64(6) <- f64[1,16] f64[1,16]", "-> np.float64[16]"],
    },
    "local_contrast.batch": {
        "*": ["srx_local_contrast_f64(6) <- f64[2,16] f64[2,16]", "-> np.float64[2,16]"],
    },
    "local_contrast_device": {
        "*": ["srx_local_contrast_f64(6) <- f64[2,16] f64[2,16]", "-> f64[2,16]"],
    },
    "radial_average": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_ring_sums_f64(10) <- f64[8,8] f64[8]", "-> (np.int64[4], np.float64[4])"],
        "t_f32 t_f32_strided": ["srx_metrics_workspace_bytes(4)", "srx_ring_sums_f32(10) <- f32[8,8] f64[8]", "-> (np.int64[4], np.float64[4])"],
    },
    "subpixel_centre": {
        "*": ["srx_spot_moments_f64(5) <- f64[8,8] f64[4]", "-> (2 x float)"],
        "t_f32 t_f32_strided": ["srx_spot_moments_f32(5) <- f32[8,8] f64[4]", "-> (2 x float)"],
    },
    "edge_magnitude": {
        "*": ["srx_metrics_workspace_bytes(4)", "srx_edge_magnitude_f64(8) <- f64[8,8] f64[8,8]", "-> f64[8,8]"],
    },
}


@pytest.mark.parametrize("case", list(CASES))
def test_wrapper_record(rec, case):
    shape, lists, fn = CASES[case]
    got = {kind: rec.take(fn, x) for kind, x in kinds(shape, lists).items()}
    want = {kind: lines for group, lines in EXPECTED[case].items() for kind in group.split()}
    want = {kind: want[kind] if kind in want else want["*"] for kind in got}
    wrong = {kind: (got[kind], want[kind]) for kind in got if got[kind] != want[kind]}
    assert not wrong, "\n".join(f"{kind}: got {g}, recorded {w}" for kind, (g, w) in wrong.items())


# -------------------------------------------------------------------------------------------------------------------------------------
# the session driver's uploads: decoded PNG files -> device frames
# -------------------------------------------------------------------------------------------------------------------------------------
def _write_files(d, names, colour=()):
    """8-bit greyscale files of 40 x 48 zeros; those named in `colour` as RGB, which load_gray's channel mean turns into float64"""
    from PIL import Image
    for n in names:
        a = np.zeros((40, 48, 3) if n in colour else (40, 48), np.uint8)
        Image.fromarray(a).save(str(d / n))
    return str(d)


def _mono_cal(tmp, **kw):
    return _write_files(tmp, [n for n, _ in session.IMAGE_SHIFTS], **kw)


def _rgb_cal(tmp, reps=(1, 1, 1, 1), **kw):
    meta = {"expected_shifts": {label: {"dy_px": 1.0, "dx_px": -1.0} for label in session.CORNER_ORDER}}
    (tmp / "metadata.json").write_text(json.dumps(meta))
    return _write_files(tmp, [f"corner{c}_rep{r:02d}.png" for c, n in enumerate(reps) for r in range(n)], **kw)


def _barcodes(tmp, **kw):
    return _write_files(tmp, [f"corner{c}_rep{r:02d}.png" for r in range(2) for c in range(4)], **kw)


def _psf_sweeps(tmp, **kw):
    for s in ("sweep0", "sweep1"):
        (tmp / s).mkdir()
        _write_files(tmp / s, ["pos4_(0,0).png"], **kw)
    return str(tmp)


def _frames(dtype, n=4, hw=(8, 8)):
    return [torch.zeros(hw, dtype=dtype) for _ in range(n)]


def _measured_psf(d):
    try:
        session.load_measured_psf_device(d)
    except FileNotFoundError:  # as in _psf
        pass


SESSION_CASES = {
    "_to_dev_f.u8": lambda tmp: session._to_dev_f(np.zeros((8, 8), np.uint8)),
    "_to_dev_f.f64": lambda tmp: session._to_dev_f(np.zeros((8, 8))),
    "_to_dev_f.f32_strided": lambda tmp: session._to_dev_f(np.zeros((8, 16), np.float32)[:, ::2]),
    "_to_dev_frames.keep_u8": lambda tmp: session._to_dev_frames([np.zeros((8, 8), np.uint8)] * 2, True),
    "_to_dev_frames.keep_u8_strided": lambda tmp: session._to_dev_frames([np.zeros((8, 16), np.uint8)[:, ::2]] * 2, True),
    "_to_dev_frames.keep_u8_one_colour_file": lambda tmp: session._to_dev_frames([np.zeros((8, 8), np.uint8), np.zeros((8, 8))], True),
    "_to_dev_frames.float": lambda tmp: session._to_dev_frames([np.zeros((8, 8), np.uint8)] * 2, False),
    "_frame_mean.u8": lambda tmp: session._frame_mean(torch.zeros((2, 4, 8, 8), dtype=torch.uint8)),
    "_frame_mean.f64": lambda tmp: session._frame_mean(torch.zeros((2, 4, 8, 8), dtype=torch.float64)),
    "load_gray_dev": lambda tmp: session.load_gray_dev(_mono_cal(tmp) + "/center.png"),
    "load_mono_cal_session": lambda tmp: session.load_mono_cal_session(_mono_cal(tmp)),
    "load_mono_cal_session.keep_u8": lambda tmp: session.load_mono_cal_session(_mono_cal(tmp), keep_u8=True),
    "load_mono_cal_session.keep_u8_one_colour_file": lambda tmp: session.load_mono_cal_session(_mono_cal(tmp, colour=("shift_1.png",)), keep_u8=True),
    "load_rgb_cal_combo": lambda tmp: session.load_rgb_cal_combo(_rgb_cal(tmp)),
    "load_rgb_cal_combo.keep_u8": lambda tmp: session.load_rgb_cal_combo(_rgb_cal(tmp, reps=(2, 2, 2, 2)), keep_u8=True),
    "load_rgb_cal_combo.keep_u8_uneven_reps": lambda tmp: session.load_rgb_cal_combo(_rgb_cal(tmp, reps=(2, 1, 2, 3)), keep_u8=True),
    "load_corner_reps": lambda tmp: session.load_corner_reps(_barcodes(tmp), red=False),
    "load_corner_reps.red": lambda tmp: session.load_corner_reps(_barcodes(tmp), red=True),
    "load_corner_reps.keep_u8": lambda tmp: session.load_corner_reps(_barcodes(tmp), red=False, keep_u8=True),
    "load_corner_reps.keep_u8_red": lambda tmp: session.load_corner_reps(_barcodes(tmp), red=True, keep_u8=True),
    "load_corner_reps.keep_u8_one_colour_file": lambda tmp: session.load_corner_reps(_barcodes(tmp, colour=("corner3_rep01.png",)), red=True, keep_u8=True),
    "load_measured_psf_device": lambda tmp: _measured_psf(_psf_sweeps(tmp)),
    "load_measured_psf_device.one_colour_file": lambda tmp: _measured_psf(_psf_sweeps(tmp, colour=("pos4_(0,0).png",))),
    "reconstruct_batch.u8_items": lambda tmp: session.reconstruct_batch([_frames(torch.uint8)] * 2, [T4, T4], PSF, 1),
    "register_shifts.u8": lambda tmp: session.register_shifts([_frames(torch.uint8, 3, (40, 40))] * 2, T3)[0][0],
    "register_shifts.f64": lambda tmp: session.register_shifts([_frames(torch.float64, 3, (40, 40))] * 2, T3)[0][0],
    "reconstruct_patchwise.u8": lambda tmp: patchwise.reconstruct_patchwise(_frames(torch.uint8, 3, (48, 48)), T3, PSF, 1, grid=grid())[:2],
}

TO_F64 = "srx_u8_to_f64(4) <- u8[40,48] f64[40,48]"
RED = "srx_decimate_f64(9) <- f64[40,48] f64[20,24]"
REP_MEAN = "srx_mean_frames_f64(6) <- f64[1,20,24] f64[20,24]"
IMAGES = "{native_2x: f32[16,16], SAA: f32[16,16], SAA_IBP: f32[16,16], LR_mean: f64[8,8]}"

SESSION_EXPECTED = {
    "_to_dev_f.u8": ["srx_u8_to_f64(4) <- u8[8,8] f64[8,8]", "-> f64[8,8]"],
    "_to_dev_f.f64": ["-> f64[8,8]"],
    "_to_dev_f.f32_strided": ["-> f64[8,8]"],
    "_to_dev_frames.keep_u8": ["-> (2 x u8[8,8])"],
    "_to_dev_frames.keep_u8_strided": ["-> (2 x u8[8,8])"],
    "_to_dev_frames.keep_u8_one_colour_file": ["srx_u8_to_f64(4) <- u8[8,8] f64[8,8]", "-> (2 x f64[8,8])"],
    "_to_dev_frames.float": ["2 x srx_u8_to_f64(4) <- u8[8,8] f64[8,8]", "-> (2 x f64[8,8])"],
    "_frame_mean.u8": ["srx_mean_u8(11) <- u8[2,4,8,8] f64[2,8,8]", "-> f64[2,8,8]"],
    "_frame_mean.f64": ["srx_mean_frames_f64(6) <- f64[2,4,8,8] f64[2,8,8]", "-> f64[2,8,8]"],
    "load_gray_dev": [TO_F64, "-> f64[40,48]"],
    "load_mono_cal_session": ["5 x " + TO_F64, "-> ((5 x f64[40,48]), (5 x (2 x float)))"],
    "load_mono_cal_session.keep_u8": ["-> ((5 x u8[40,48]), (5 x (2 x float)))"],
    "load_mono_cal_session.keep_u8_one_colour_file": ["4 x " + TO_F64, "-> ((5 x f64[40,48]), (5 x (2 x float)))"],
    "load_rgb_cal_combo": 4 * [TO_F64, RED, REP_MEAN] + ["-> ((4 x f64[20,24]), (4 x (2 x float)))"],
    "load_rgb_cal_combo.keep_u8": ["srx_mean_u8(11) <- u8[4,2,40,48] f64[4,20,24]", "-> ((4 x f64[20,24]), (4 x (2 x float)))"],
    "load_rgb_cal_combo.keep_u8_uneven_reps":
        ["srx_mean_u8(11) <- u8[1,2,40,48] f64[1,20,24]",
         "srx_mean_u8(11) <- u8[1,1,40,48] f64[1,20,24]",
         "srx_mean_u8(11) <- u8[1,2,40,48] f64[1,20,24]",
         "srx_mean_u8(11) <- u8[1,3,40,48] f64[1,20,24]",
         "-> ((4 x f64[20,24]), (4 x (2 x float)))"],
    "load_corner_reps": ["8 x " + TO_F64, "-> ((2 x (4 x f64[40,48])), (4 x (2 x float)))"],
    "load_corner_reps.red": ["4 x " + TO_F64, "4 x " + RED, "4 x " + TO_F64, "4 x " + RED, "-> ((2 x (4 x f64[20,24])), (4 x (2 x float)))"],
    "load_corner_reps.keep_u8": ["-> ((2 x (4 x u8[40,48])), (4 x (2 x float)))"],
    "load_corner_reps.keep_u8_red": ["8 x srx_decimate_u8(9) <- u8[1,40,48] u8[1,20,24]", "-> ((2 x (4 x u8[20,24])), (4 x (2 x float)))"],
    "load_corner_reps.keep_u8_one_colour_file":
        ["4 x " + TO_F64, "4 x " + RED, "3 x " + TO_F64, "4 x " + RED, "-> ((2 x (4 x f64[20,24])), (4 x (2 x float)))"],
    "load_measured_psf_device": ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_u8(10) <- u8[2,40,48] f64[7,7] i32[2,3]", "-> NoneType"],
    "load_measured_psf_device.one_colour_file":
        ["srx_psf_estimate_workspace_bytes(5)", "srx_psf_estimate_f64(10) <- f64[2,40,48] f64[7,7] i32[2,3]", "-> NoneType"],
    "reconstruct_batch.u8_items":
        ["srx_mean_u8(11) <- u8[2,4,8,8] f64[2,8,8]",
         "srx_zoom_workspace_bytes(5)",
         "srx_zoom_cubic_f32(9) <- f32[2,8,8] f32[2,16,16]",
         "srx_u8_to_f32(4) <- u8[2,4,8,8] f32[2,4,8,8]",
         "srx_saa_items_workspace_bytes(6)",
         "srx_saa_items_f32(12) <- f32[2,4,8,8] f32[2,16,16]",
         "srx_u8_to_f32(4) <- u8[2,4,8,8] f32[2,4,8,8]",
         "srx_ibp_items_workspace_bytes_for(13)",
         "srx_ibp_items_f32(21) <- f32[2,4,8,8] f32[2,16,16] f32[2,16,16] f64[2,1]",
         "-> (2 x (" + IMAGES + ", (float)))"],
    "register_shifts.u8": ["srx_register_workspace_bytes(6)", "srx_register_u8_f32(17) <- u8[2,3,40,40] f64[2,3,2] f64[2,3] i32[2,3]", "-> (3 x (2 x float))"],
    "register_shifts.f64": ["srx_register_workspace_bytes(6)", "srx_register_f32(17) <- f32[2,3,40,40] f64[2,3,2] f64[2,3] i32[2,3]", "-> (3 x (2 x float))"],
    "reconstruct_patchwise.u8":
        ["srx_mean_u8(11) <- u8[1,3,48,48] f64[1,48,48]",
         "srx_zoom_workspace_bytes(5)",
         "srx_zoom_cubic_f32(9) <- f32[1,48,48] f32[1,96,96]",
         "srx_patches_gather_u8(11) <- u8[1,3,48,48] u8[4,3,40,40]",
         "srx_register_workspace_bytes(6)",
         "srx_register_u8_f32(17) <- u8[4,3,40,40] f64[4,3,2] f64[4,3] i32[4,3]",
         "srx_u8_to_f32(4) <- u8[4,3,40,40] f32[4,3,40,40]",
         "srx_saa_items_workspace_bytes(6)",
         "srx_saa_items_f32(12) <- f32[4,3,40,40] f32[4,80,80]",
         "srx_u8_to_f32(4) <- u8[4,3,40,40] f32[4,3,40,40]",
         "srx_ibp_items_workspace_bytes_for(13)",
         "srx_ibp_items_f32(21) <- f32[4,3,40,40] f32[4,80,80] f32[4,80,80] f64[4,1]",
         "2 x srx_patches_blend_f32(11) <- f32[4,80,80] f32[1,96,96]",
         "-> ({native_2x: f32[96,96], SAA: f32[96,96], SAA_IBP: f32[96,96], LR_mean: f64[48,48]}, (float))"],
}


@pytest.mark.parametrize("case", list(SESSION_CASES))
def test_session_record(rec, tmp_path, case):
    assert rec.take(SESSION_CASES[case], tmp_path) == SESSION_EXPECTED[case]


def test_every_rejection_comes_before_the_device(monkeypatch):
    """The rejecting inputs of the uint8-only wrappers, once more with a device that must not be asked for"""
    def no_device(*a, **k):
        raise AssertionError("the wrapper touched the device before checking its arguments")

    monkeypatch.setattr(api, "_device", no_device)
    f32, k = np.zeros((1, 4, 8, 8), np.float32), torch.zeros((1, 4, 8, 8), dtype=torch.int16)
    for bad in (f32, k):
        for fn in (lambda x: api.shift_and_add_u8_batched(x, T4, 2), lambda x: api.ibp_u8_batched(x, T4, PSF, HR0, 2, 1), api.mean_u8,
                   lambda x: api.decimate_u8(x[0], 2)):
            with pytest.raises(TypeError):
                fn(bad)
        with pytest.raises(ValueError):
            api.crc32(bad[0, 0])
    with pytest.raises(ValueError):
        api.crc32(np.zeros((2, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        api.decimate_u8(np.zeros((1, 2, 8, 8), np.uint8), 2)
    with pytest.raises(TypeError):
        patchwise.blend(np.zeros((4, 80, 80), np.uint8), grid())
    with pytest.raises(TypeError):
        patchwise.gather(torch.zeros((4, 48, 48), dtype=torch.int16), grid())
