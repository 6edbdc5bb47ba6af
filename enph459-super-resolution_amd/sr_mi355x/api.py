"""Host-side mirror of the reference's SR core on top of libsrx.so (HIP, gfx950).

Same names, argument order and meaning as the module-level functions of the reference's
drivers (mono_cal_target/run_sr.py:157-209; identical in the other three run_sr.py):

    blur(img, kernel)                                              :157-158
    forward_model(hr, kernel, shift_yx, factor)                    :161-165
    back_project(error_lr, kernel, shift_yx, factor, hr_shape)     :168-178
    shift_and_add(lr_list, shifts_yx, factor=2, order=3)           :181-187
    ibp(lr_list, shifts_yx, kernel, hr_init, factor=2, n_iter=80, step=0.5) -> (hr, errors)   :190-209
    ndi_zoom(img, factor, order=3) / ndi_shift(img, shift, order=3, mode='nearest')  (the two SciPy
        calls the drivers make directly, :279 and :163)

so `from sr_mi355x import ibp, shift_and_add, ...` (or rebinding those names in a run_sr
module) makes the reference's own process_session run on the MI355X.  numpy in -> float64
numpy out (like the reference); torch CUDA tensors in -> torch tensors out, no host copy.
`*_batched` variants take a leading batch of independent work items (patches, sessions x reps).

Compute precision: 'f32' (default; HBM-bound fast path, |delta| ~ 2e-4 DN vs float64) or
'f64' (the reference's own precision, ~1e-10 DN).  torch is only plumbing here (device
memory + streams); every FLOP runs in libsrx.so, and there is no CPU fallback.
"""
import ctypes
import os
import threading

import numpy as np
import torch

from . import _lib
from ._lib import (FLAG_AUTO, FLAG_COMPOSED, FLAG_FUSED, FLAG_PER_FRAME, FLAG_TILES, FLAG_DIAG_NO_ZERO_FUSE,  # noqa: F401  (re-exported)
                   FLAG_DIAG_NO_SEPARABLE, FLAG_DIAG_NO_PREFILTER_TILE, FLAG_DIAG_V1, FLAG_DIAG_WIDE_WINDOWS, FLAG_DIAG_COLUMN_TILES,
                   FLAG_DIAG_TWO_LAUNCH, FLAG_DIAG_SAA_ONE_PASS, FLAG_DIAG_U8_BYTE_LOADS)

_TORCH_DT = {"f32": torch.float32, "f64": torch.float64}
_ELEM = {"f32": 4, "f64": 8}
# The working precision is a per-THREAD setting with a process-wide default: the session driver's loader thread works in float64
# (precision_override) while the main thread reconstructs in float32, and neither may see the other's choice.
_DEFAULT_PRECISION = "f32"
_tls = threading.local()


def set_precision(p):
    """'f32' or 'f64': element type of every device buffer and of the arithmetic.  Sets the process default (what every thread
    uses unless it is inside a precision_override) and drops the calling thread's override, if any."""
    global _DEFAULT_PRECISION
    if p not in _TORCH_DT:
        raise ValueError("precision must be 'f32' or 'f64'")
    _DEFAULT_PRECISION = p
    _tls.p = None


def get_precision():
    return getattr(_tls, "p", None) or _DEFAULT_PRECISION


class precision_override:
    """with precision_override('f64'): ... -- the calling thread's precision inside the block, other threads untouched."""

    def __init__(self, p):
        if p not in _TORCH_DT:
            raise ValueError("precision must be 'f32' or 'f64'")
        self.p = p

    def __enter__(self):
        self.prev = getattr(_tls, "p", None)
        _tls.p = self.p

    def __exit__(self, *exc):
        _tls.p = self.prev


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("sr_mi355x needs an MI355X (HIP device); there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _to_dev(x, prec=None, *, allowed=None, as_is=(np.uint8,), what="input", error=TypeError):
    """The one path from caller data to the device: tensor or array -> (contiguous CUDA tensor, was_numpy).
    prec: 'f32' / 'f64' or a torch dtype, what the data is cast to ON THE DEVICE; None keeps the dtype, which must then be one of
    `allowed` (None: any) or `error` is raised naming `what`.  as_is: the dtypes of host arrays that are uploaded as they are and cast
    on the device; any other host array is widened to float64 on the host first.  None: every array is handed to torch as it is, like a
    tensor (a cast to `prec` then comes before the upload).  The dtype is checked before the device is touched."""
    dt = _TORCH_DT.get(prec, prec)
    was_numpy = not isinstance(x, torch.Tensor)
    if was_numpy:
        a = np.ascontiguousarray(np.asarray(x))
        if as_is is not None and a.dtype not in as_is:
            a = a.astype(np.float64, copy=False)
        x = torch.from_numpy(a)
    if dt is None and allowed is not None and x.dtype not in allowed:
        raise error(f"{what} must be one of {[str(d) for d in allowed]}, not {x.dtype}")
    if was_numpy and as_is is not None:
        x = x.to(device=_device())
    return x.to(device=_device(), dtype=dt).contiguous(), was_numpy


_BYTES = {"allowed": (torch.uint8,), "as_is": None}  # _to_dev's policy for the camera's samples: uint8 only, uploaded as bytes, never cast


def _stack_dev(lst, prec=None, **policy):
    """_to_dev of a stack of frames: a tensor or an array as it is, a sequence of tensors stacked on the device, any other sequence as
    one host array (np.stack: a ValueError for frames of different shapes and for no frames, an empty array included)"""
    if isinstance(lst, torch.Tensor) or isinstance(lst, np.ndarray) and len(lst):
        return _to_dev(lst, prec, **policy)
    if len(lst) and isinstance(lst[0], torch.Tensor):
        return _to_dev(torch.stack([t.to(device=_device(), dtype=_TORCH_DT.get(prec, prec)) for t in lst]), prec, **policy)[0], False
    return _to_dev(np.stack([np.asarray(a) for a in lst]), prec, **policy)


def _is_u8(x):
    """x, or every frame of the sequence x, is a uint8 tensor or array (a plain list of numbers is not): what goes to the library as bytes"""
    def u8(a):
        return isinstance(a, (torch.Tensor, np.ndarray)) and a.dtype == (torch.uint8 if isinstance(a, torch.Tensor) else np.uint8)
    return u8(x) if isinstance(x, (torch.Tensor, np.ndarray)) else len(x) > 0 and all(u8(f) for f in x)


def _batch(x, ndim):
    """x [...] of rank ndim - 1 or ndim -> (x with the optional leading batch axis, whether it had to be added); _unbatch takes it off again"""
    single = x.dim() == ndim - 1
    return (x[None] if single else x), single


def _unbatch(out, single, was_numpy=False):
    out = out[0] if single else out
    return out.cpu().numpy() if was_numpy else out


def _out(t, was_numpy):
    return t.to(torch.float64).cpu().numpy() if was_numpy else t


def _host_f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a, a.ctypes.data_as(_lib._HD)


def _shape4(x, what):
    """(B, N, h, w) of a frame stack before it is moved anywhere"""
    shp = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
    if len(shp) != 4:
        raise ValueError(f"{what} must have 4 dimensions [B, N, h, w]")
    return tuple(int(v) for v in shp)


def _shift_tables(shifts_yx, B, N):
    """shifts_yx [N, 2] (one table shared by the batch) or [B, N, 2] (one per item: the *_items_* entry points) ->
    (array, ctypes pointer, per_item); any other shape is a ValueError."""
    a = np.ascontiguousarray(np.asarray(shifts_yx, dtype=np.float64))
    if a.shape == (N, 2):
        return a, a.ctypes.data_as(_lib._HD), False
    if a.shape == (B, N, 2):
        return a, a.ctypes.data_as(_lib._HD), True
    raise ValueError(f"shifts_yx must have shape {(N, 2)} or {(B, N, 2)}, not {a.shape}")


def _ws(nbytes):
    t = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=_device())
    return t, ctypes.c_void_p(t.data_ptr()), ctypes.c_size_t(t.numel())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _fn(name, prec):
    return getattr(_lib.load(), f"{name}_{prec}")


def last_path():
    """The name of the code path the last shift_and_add / ibp call on this thread took (include/srx.h, srx_last_path): 'mosaic', 'fused',
    'composed', ibp's kernel names such as 'patch' or 'btile', or 'mixed' after a per-item call whose runs took different ones."""
    return _lib.load().srx_last_path().decode()


# ------------------------------------------------------------------------------------------
# batched primitives: tensors [B, ...] on the device
# ------------------------------------------------------------------------------------------
def blur_batched(img, kernel, precision=None):
    prec = precision or get_precision()
    x, _ = _to_dev(img, prec)
    B, H, W = x.shape
    k, kp = _host_f64(kernel)
    out = torch.empty_like(x)
    _lib.check(_fn("srx_blur", prec)(_p(x), B, H, W, kp, k.shape[0], k.shape[1], _p(out), _stream()), "srx_blur")
    return out


def shift_batched(img, shift_yx, precision=None):
    prec = precision or get_precision()
    x, _ = _to_dev(img, prec)
    B, H, W = x.shape
    out = torch.empty_like(x)
    wt, wp, wn = _ws(_lib.load().srx_shift_workspace_bytes(_ELEM[prec], B, H, W))
    _lib.check(_fn("srx_shift_cubic", prec)(_p(x), B, H, W, float(shift_yx[0]), float(shift_yx[1]), _p(out), wp, wn,
                                            _stream()), "srx_shift_cubic")
    return out


def zoom_batched(img, factor, precision=None):
    prec = precision or get_precision()
    x, _ = _to_dev(img, prec)
    B, h, w = x.shape
    f = int(factor)
    if f != factor or f < 1:
        raise ValueError("zoom factor must be a positive integer")
    out = torch.empty((B, h * f, w * f), dtype=x.dtype, device=x.device)
    wt, wp, wn = _ws(_lib.load().srx_zoom_workspace_bytes(_ELEM[prec], B, h, w, f))
    _lib.check(_fn("srx_zoom_cubic", prec)(_p(x), B, h, w, f, _p(out), wp, wn, _stream()), "srx_zoom_cubic")
    return out


def forward_model_batched(hr, kernel, shift_yx, factor, precision=None):
    prec = precision or get_precision()
    x, _ = _to_dev(hr, prec)
    B, H, W = x.shape
    f = int(factor)
    k, kp = _host_f64(kernel)
    out = torch.empty((B, -(-H // f), -(-W // f)), dtype=x.dtype, device=x.device)
    wt, wp, wn = _ws(_lib.load().srx_forward_workspace_bytes(_ELEM[prec], B, H, W))
    _lib.check(_fn("srx_forward", prec)(_p(x), B, H, W, kp, k.shape[0], k.shape[1], float(shift_yx[0]),
                                        float(shift_yx[1]), f, _p(out), wp, wn, _stream()), "srx_forward")
    return out


def back_project_batched(error_lr, kernel, shift_yx, factor, hr_shape, precision=None):
    prec = precision or get_precision()
    e, _ = _to_dev(error_lr, prec)
    B, eh, ew = e.shape
    H, W = int(hr_shape[0]), int(hr_shape[1])
    k, kp = _host_f64(kernel)
    out = torch.empty((B, H, W), dtype=e.dtype, device=e.device)
    wt, wp, wn = _ws(_lib.load().srx_backproject_workspace_bytes(_ELEM[prec], B, H, W))
    _lib.check(_fn("srx_backproject", prec)(_p(e), B, eh, ew, kp, k.shape[0], k.shape[1], float(shift_yx[0]),
                                            float(shift_yx[1]), int(factor), H, W, _p(out), wp, wn, _stream()),
               "srx_backproject")
    return out


def _saa_batched(lr, u8, shifts_yx, factor, precision, flags):
    """the body of shift_and_add_batched and, with u8 (the frames are and stay bytes), of shift_and_add_u8_batched"""
    prec, what = precision or get_precision(), "lr_u8" if u8 else "lr"
    B, N, h, w = _shape4(lr, what)
    sh, shp, per_item = _shift_tables(shifts_yx, B, N)
    x = _to_dev(lr, what=what, **_BYTES)[0] if u8 else _to_dev(lr, prec)[0]
    if u8 and per_item:  # no uint8 items entry point: the frames are converted on the device ((T)uint8 is exact: the same bits)
        return _saa_batched(u8_to_float(x, prec), False, sh, factor, prec, flags)
    f = int(factor)
    out = torch.empty((B, h * f, w * f), dtype=_TORCH_DT[prec], device=x.device)
    name = "srx_saa_u8lr" if u8 else "srx_saa_items" if per_item else "srx_saa"
    wt, wp, wn = _ws(getattr(_lib.load(), name + "_workspace_bytes")(_ELEM[prec], B, N, h, w, f))
    _lib.check(_fn(name, prec)(_p(x), B, N, h, w, shp, f, _p(out), wp, wn, _stream(), flags), name)
    return out


def shift_and_add_batched(lr, shifts_yx, factor=2, precision=None, flags=FLAG_AUTO):
    """lr [B, N, h, w] -> [B, h*f, w*f].  shifts_yx [N, 2], or [B, N, 2] for one table per item (srx_saa_items_*)."""
    return _saa_batched(lr, False, shifts_yx, factor, precision, flags)


def shift_and_add_u8_batched(lr_u8, shifts_yx, factor=2, precision=None, flags=FLAG_AUTO):
    """shift_and_add_batched on the camera's own samples: lr_u8 uint8 [B, N, h, w] -> [B, h*f, w*f] of the compute precision; the same
    bits as shift_and_add_batched on the converted frames (srx_saa_u8lr_*)."""
    return _saa_batched(lr_u8, True, shifts_yx, factor, precision, flags)


def _ibp_batched(lr, u8, shifts_yx, kernel, hr_init, factor, n_iter, step, precision, flags, want_errors, out, exact_workspace):
    """the body of ibp_batched and, with u8 (the frames are and stay bytes), of ibp_u8_batched"""
    prec, what = precision or get_precision(), "lr_u8" if u8 else "lr"
    B, N, h, w = _shape4(lr, what)
    sh, shp, per_item = _shift_tables(shifts_yx, B, N)
    x = _to_dev(lr, what=what, **_BYTES)[0] if u8 else _to_dev(lr, prec)[0]
    if u8 and per_item:  # as in _saa_batched
        return _ibp_batched(u8_to_float(x, prec), False, sh, kernel, hr_init, factor, n_iter, step, prec, flags, want_errors, out, exact_workspace)
    h0, _ = _to_dev(hr_init, prec)
    Bh, H, W = h0.shape
    if Bh != B:
        raise ValueError(f"{what} and hr_init disagree on the batch size")
    f = int(factor)
    k, kp = _host_f64(kernel)
    name = "srx_ibp_u8lr" if u8 else "srx_ibp_items" if per_item else "srx_ibp"
    if out is not None:  # the library writes B*H*W elements of the call's precision straight through this pointer
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != _TORCH_DT[prec] or tuple(out.shape) != (B, H, W)
                or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous CUDA tensor of dtype {_TORCH_DT[prec]} and shape {(B, H, W)}")
    hr = torch.empty_like(h0) if out is None else out
    errors = torch.empty((B, int(n_iter)), dtype=torch.float64, device=x.device) if want_errors else None
    lib = _lib.load()
    wt, wp, wn = _ws(getattr(lib, name + "_workspace_bytes_for")(_ELEM[prec], B, N, h, w, H, W, f, shp, kp, k.shape[0], k.shape[1], flags)
                     if exact_workspace else getattr(lib, name + "_workspace_bytes")(_ELEM[prec], B, N, h, w, H, W, f, flags))
    _lib.check(_fn(name, prec)(_p(x), B, N, h, w, shp, kp, k.shape[0], k.shape[1], _p(h0), H, W, f, int(n_iter),
                               float(step), _p(hr), _p(errors) if want_errors else None, wp, wn, _stream(), flags),
               name)
    return hr, errors


def ibp_batched(lr, shifts_yx, kernel, hr_init, factor=2, n_iter=80, step=0.5, precision=None, flags=FLAG_AUTO,
                want_errors=True, out=None, exact_workspace=True):
    """lr [B, N, h, w], hr_init [B, H, W] -> (hr [B, H, W], errors float64 [B, n_iter] or None).
    `exact_workspace=False` sizes the arena by the shape-only bound (srx_ibp_workspace_bytes), as a caller without the shift table
    at hand would.  shifts_yx [N, 2], or [B, N, 2] for one table per item (srx_ibp_items_*: item b gets the bits of a B = 1 call
    on shifts_yx[b])."""
    return _ibp_batched(lr, False, shifts_yx, kernel, hr_init, factor, n_iter, step, precision, flags, want_errors, out, exact_workspace)


def ibp_u8_batched(lr_u8, shifts_yx, kernel, hr_init, factor=2, n_iter=80, step=0.5, precision=None, flags=FLAG_AUTO,
                   want_errors=True, out=None, exact_workspace=True):
    """ibp_batched on the camera's own samples: lr_u8 uint8 [B, N, h, w], hr_init [B, H, W] -> (hr, errors); the same bits as
    ibp_batched on the converted frames (srx_ibp_u8lr_*)."""
    return _ibp_batched(lr_u8, True, shifts_yx, kernel, hr_init, factor, n_iter, step, precision, flags, want_errors, out, exact_workspace)


class IbpPlan:
    """srx_ibp_plan_* (include/srx.h): the IBP loop of a batch in instalments -- the per-call tables built once, `run(n)` for n more
    iterations, rows of the state readable / replaceable in between.  `trace_rows=(lo, hi)`: the HR rows whose LR samples the MSE trace
    counts (a row band of a larger image counts its own rows only; `supports_trace_rows` says whether this plan can).  The tensors
    passed in and the workspace live as long as the plan."""

    def __init__(self, lr, shifts_yx, kernel, hr_init, factor=2, step=0.5, precision=None, flags=FLAG_AUTO, trace_rows=None):
        self.prec = precision or get_precision()
        self.lr, _ = _to_dev(lr, self.prec)
        h0, _ = _to_dev(hr_init, self.prec)
        self.B, self.N, self.h, self.w = self.lr.shape
        _, self.H, self.W = h0.shape
        self._sh = _host_f64(shifts_yx, (self.N, 2))
        self._k = _host_f64(kernel)
        lo, hi = trace_rows if trace_rows is not None else (0, self.H)
        lib = _lib.load()
        self._ws = _ws(lib.srx_ibp_plan_workspace_bytes(_ELEM[self.prec], self.B, self.N, self.h, self.w, self.H, self.W, int(factor), flags))
        self._h = ctypes.c_void_p()
        k = self._k[0]
        _lib.check(_fn("srx_ibp_plan_create", self.prec)(_p(self.lr), self.B, self.N, self.h, self.w, self._sh[1], self._k[1], k.shape[0], k.shape[1],
                                                         _p(h0), self.H, self.W, int(factor), float(step), int(lo), int(hi), self._ws[1], self._ws[2],
                                                         _stream(), flags, ctypes.byref(self._h)), "srx_ibp_plan_create")
        self.path = lib.srx_ibp_plan_path(self._h).decode()
        self.supports_trace_rows = bool(lib.srx_ibp_plan_supports_trace_rows(self._h))

    def run(self, n_iter, want_errors=True):
        """n more iterations -> errors float64 [B, n] on the device (this run's slice of the trace) or None"""
        errors = torch.empty((self.B, int(n_iter)), dtype=torch.float64, device=self.lr.device) if want_errors and n_iter > 0 else None
        _lib.check(_lib.load().srx_ibp_plan_run(self._h, int(n_iter), _p(errors) if errors is not None else None, _stream()), "srx_ibp_plan_run")
        return errors

    def get_rows(self, lo, hi, out=None):
        out = torch.empty((self.B, hi - lo, self.W), dtype=_TORCH_DT[self.prec], device=self.lr.device) if out is None else out
        _lib.check(_fn("srx_ibp_plan_get_rows", self.prec)(self._h, int(lo), int(hi), _p(out), _stream()), "srx_ibp_plan_get_rows")
        return out

    def set_rows(self, lo, hi, rows):
        rows = rows.to(device=self.lr.device, dtype=_TORCH_DT[self.prec]).contiguous()
        if tuple(rows.shape) != (self.B, hi - lo, self.W):
            raise ValueError(f"rows must have shape {(self.B, hi - lo, self.W)}")
        _lib.check(_fn("srx_ibp_plan_set_rows", self.prec)(self._h, int(lo), int(hi), _p(rows), _stream()), "srx_ibp_plan_set_rows")

    def result(self):
        return self.get_rows(0, self.H)

    def close(self):
        if self._h:
            _lib.load().srx_ibp_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# the reference's call surface (single image; numpy or torch)
# ------------------------------------------------------------------------------------------
def blur(img, kernel):
    x, was_np = _to_dev(img, get_precision())
    return _out(blur_batched(x[None], kernel)[0], was_np)


def ndi_shift(img, shift, order=3, mode="nearest"):
    if order != 3 or mode != "nearest":
        raise NotImplementedError("only order=3, mode='nearest' (the reference's call) is provided")
    x, was_np = _to_dev(img, get_precision())
    return _out(shift_batched(x[None], shift)[0], was_np)


def ndi_zoom(img, zoom, order=3):
    if order != 3:
        raise NotImplementedError("only order=3 (the reference's call) is provided")
    x, was_np = _to_dev(img, get_precision())
    return _out(zoom_batched(x[None], zoom)[0], was_np)


def forward_model(hr, kernel, shift_yx, factor):
    x, was_np = _to_dev(hr, get_precision())
    return _out(forward_model_batched(x[None], kernel, shift_yx, factor)[0], was_np)


def back_project(error_lr, kernel, shift_yx, factor, hr_shape):
    x, was_np = _to_dev(error_lr, get_precision())
    return _out(back_project_batched(x[None], kernel, shift_yx, factor, hr_shape)[0], was_np)


def shift_and_add(lr_list, shifts_yx, factor=2, order=3):
    if order != 3:
        raise NotImplementedError("only order=3 (the reference's call) is provided")
    x, was_np = _stack_dev(lr_list, get_precision())
    return _out(shift_and_add_batched(x[None], shifts_yx, factor)[0], was_np)


def ibp(lr_list, shifts_yx, kernel, hr_init, factor=2, n_iter=80, step=0.5, verbose=True):
    """Returns (hr, errors) like run_sr.py:190-209; `errors` is a list of n_iter floats."""
    x, was_np = _stack_dev(lr_list, get_precision())
    h0, was_np_h = _to_dev(hr_init, get_precision())
    hr, errs = ibp_batched(x[None], shifts_yx, kernel, h0[None], factor, n_iter, step)
    errors = [float(e) for e in errs[0].cpu().numpy()]
    if verbose:  # the reference prints the running MSE every 10 iterations (:207-208)
        for it in range(9, len(errors), 10):
            print(f"    iter {it + 1:3d}/{n_iter}  MSE = {errors[it]:.4f}")
    return _out(hr[0], was_np or was_np_h), errors


# ------------------------------------------------------------------------------------------
# driver glue (index maps, loaders' arithmetic, quantiser)
# ------------------------------------------------------------------------------------------
def decimate(img, f, py=0, px=0):
    """img[py::f, px::f] (run_sr.py:165)."""
    x, was_np = _to_dev(img, get_precision())
    H, W = x.shape
    out = torch.empty((-(-(H - py) // f), -(-(W - px) // f)), dtype=x.dtype, device=x.device)
    _lib.check(_fn("srx_decimate", get_precision())(_p(x), 1, H, W, int(f), int(py), int(px), _p(out), _stream()),
               "srx_decimate")
    return _out(out, was_np)


def extract_red(img):
    """Bayer RGGB red plane img[0::2, 0::2] (rgb_cal_target/run_sr.py:73-75)."""
    return decimate(img, 2, 0, 0)


def decimate_u8(img_u8, f, py=0, px=0):
    """img[..., py::f, px::f] on bytes: uint8 [H, W] or [B, H, W] -> uint8 (srx_decimate_u8); numpy in -> numpy out."""
    if np.ndim(img_u8) not in (2, 3):
        raise ValueError("img_u8 must be [H, W] or [B, H, W]")
    x, was_np = _to_dev(img_u8, what="img_u8", **_BYTES)
    x, single = _batch(x, 3)
    B, H, W = x.shape
    out = torch.empty((B, -(-(H - py) // f), -(-(W - px) // f)), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().srx_decimate_u8(_p(x), B, H, W, int(f), int(py), int(px), _p(out), _stream()), "srx_decimate_u8")
    return _unbatch(out, single, was_np)


def extract_red_u8(img_u8):
    """Bayer RGGB red plane of a raw uint8 frame, kept in bytes (rgb_cal_target/run_sr.py:73-75 without the cast)."""
    return decimate_u8(img_u8, 2, 0, 0)


def zero_insert(err, f, hr_shape):
    """up = zeros(hr_shape); up[::f, ::f] = err (pad/crop) (run_sr.py:170-175)."""
    x, was_np = _to_dev(err, get_precision())
    eh, ew = x.shape
    H, W = int(hr_shape[0]), int(hr_shape[1])
    out = torch.empty((H, W), dtype=x.dtype, device=x.device)
    _lib.check(_fn("srx_zero_insert", get_precision())(_p(x), 1, eh, ew, int(f), H, W, _p(out), _stream()),
               "srx_zero_insert")
    return _out(out, was_np)


def mean_frames(stack):
    """np.mean(stack, axis=0) (run_sr.py:274; rgb_cal_target/run_sr.py:107-108)."""
    x, was_np = _stack_dev(stack, get_precision())
    R = x.shape[0]
    n = x[0].numel()
    out = torch.empty(x.shape[1:], dtype=x.dtype, device=x.device)
    _lib.check(_fn("srx_mean_frames", get_precision())(_p(x), 1, R, n, _p(out), _stream()), "srx_mean_frames")
    return _out(out, was_np)


def mean_frames_batched(stacks):
    """[B, R, ...] -> [B, ...]: np.mean(axis=0) of every item's stack in one call."""
    x, was_np = _to_dev(stacks, get_precision())
    B, R = x.shape[0], x.shape[1]
    n = x[0, 0].numel()
    out = torch.empty((B,) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    _lib.check(_fn("srx_mean_frames", get_precision())(_p(x), B, R, n, _p(out), _stream()), "srx_mean_frames")
    return _out(out, was_np)


def mean_u8(stack_u8, f=1, py=0, px=0, precision=None):
    """The mean over R uint8 frames of the samples at [py::f, px::f]: uint8 [B, R, H, W] -> device tensor [B, h, w] of the compute
    precision (srx_mean_u8).  f=2 is the rep mean of the Bayer red planes (rgb_cal_target/run_sr.py:73-75, 107-108), f=1
    np.mean(lr_frames, 0) (run_sr.py:274); the same bits as mean_frames_batched on decimate on u8_to_float, without the float frames."""
    prec = precision or get_precision()
    B, R, H, W = _shape4(stack_u8, "stack_u8")
    x, _ = _to_dev(stack_u8, what="stack_u8", **_BYTES)
    f, py, px = int(f), int(py), int(px)
    if f <= 0 or not (0 <= py < H and 0 <= px < W):
        raise ValueError("mean_u8 needs f > 0, 0 <= py < H and 0 <= px < W")
    out = torch.empty((B, -(-(H - py) // f), -(-(W - px) // f)), dtype=_TORCH_DT[prec], device=x.device)
    _lib.check(_lib.load().srx_mean_u8(_p(x), B, R, H, W, f, py, px, _ELEM[prec], _p(out), _stream()), "srx_mean_u8")
    return out


def quantize_u8(img):
    """np.clip(img, 0, 255).astype(np.uint8): clamp, then truncate (run_sr.py:303)."""
    x, was_np = _to_dev(img, get_precision())
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _lib.check(_fn("srx_quantize_u8", get_precision())(_p(x), x.numel(), _p(out), _stream()), "srx_quantize_u8")
    return out.cpu().numpy() if was_np else out


def png_deflate(images):
    """The zlib streams of the 8-bit greyscale PNGs of `images` (srx_png_deflate_*): a [B, H, W] or [H, W] tensor / array, uint8 or float.
    Float images are quantised as quantize_u8 does (the working precision's arithmetic) while they are read; no uint8 plane is made.
    -> (streams uint8 [B, srx_png_stream_bound(H, W)], lengths int64 [B]) on the device, nothing synchronised: bytes [0, lengths[b]) of
    row b inflate to the Up-filtered scanlines of image b, and session.png_container(W, H, those bytes) is the file."""
    x, kind = _png_input(images)
    B, H, W = (int(v) for v in x.shape)
    lib = _lib.load()
    streams = torch.empty((B, lib.srx_png_stream_bound(H, W)), dtype=torch.uint8, device=x.device)
    lengths = torch.empty((B,), dtype=torch.int64, device=x.device)
    ws, wsp, wsn = _ws(lib.srx_png_scratch_bytes(B, H, W))
    _lib.check(getattr(lib, "srx_png_deflate_" + kind)(_p(x), B, H, W, _p(streams), _p(lengths), wsp, wsn, _stream()), "srx_png_deflate")
    return streams, lengths


def _png_input(images):
    """-> (device tensor [B, H, W], the entry points' suffix): uint8 stays bytes, anything else becomes the working precision"""
    kind = "u8" if _is_u8(images) else get_precision()
    x, _ = _batch(_to_dev(images, None if kind == "u8" else kind)[0], 3)
    if x.dim() != 3:
        raise ValueError("images must have the shape [B, H, W] or [H, W]")
    return x, kind


def png_file(images):
    """The 8-bit greyscale PNG files of `images` (srx_png_file_*; png_deflate's argument), complete on the device: signature, IHDR, one IDAT
    around png_deflate's stream with its CRC-32, IEND.
    -> (files uint8 [B, srx_png_file_bound(H, W)], lengths int64 [B]) on the device, nothing synchronised: bytes [0, lengths[b]) of row b
    are the file of image b, the bytes session.png_container(W, H, png_deflate's stream) would be."""
    x, kind = _png_input(images)
    B, H, W = (int(v) for v in x.shape)
    lib = _lib.load()
    files = torch.empty((B, lib.srx_png_file_bound(H, W)), dtype=torch.uint8, device=x.device)
    lengths = torch.empty((B,), dtype=torch.int64, device=x.device)
    ws, wsp, wsn = _ws(lib.srx_png_file_scratch_bytes(B, H, W))
    _lib.check(getattr(lib, "srx_png_file_" + kind)(_p(x), B, H, W, _p(files), _p(lengths), wsp, wsn, _stream()), "srx_png_file")
    return files, lengths


def png_encode(images):
    """-> a list of bytes, one complete PNG file per image of `images` (png_deflate's argument): png_file's slots, downloaded and cut to
    their lengths.  A convenience: it synchronises."""
    files, lengths = png_file(images)
    host, n = files.cpu().numpy(), lengths.cpu().tolist()
    return [host[b, :n[b]].tobytes() for b in range(len(n))]


def crc32(data, lengths=None, seed=0):
    """zlib.crc32 of device buffers (srx_crc32): `data` a [B, n] or [n] uint8 tensor / array, item b its row's first min(lengths[b], n) bytes
    (lengths: int64 [B] tensor / array, read on the device; None: whole rows), `seed` as in zlib.crc32(item, seed).
    -> int64 device tensor [B], values in [0, 2^32); nothing is synchronised."""
    if np.ndim(data) not in (1, 2):
        raise ValueError("data must have the shape [B, n] or [n]")
    x, _ = _batch(_to_dev(data, what="data", error=ValueError, **_BYTES)[0], 2)
    B, n = (int(v) for v in x.shape)
    seed = int(seed)
    if B <= 0 or not 0 <= seed < (1 << 32):
        raise ValueError("crc32 needs at least one item and a seed in [0, 2^32)")
    if lengths is not None:
        lengths = (lengths if isinstance(lengths, torch.Tensor) else torch.from_numpy(np.asarray(lengths, dtype=np.int64)))
        lengths = lengths.to(device=x.device, dtype=torch.int64).contiguous()
        if tuple(lengths.shape) != (B,):
            raise ValueError("lengths must have the shape [B]")
    if n == 0:  # no byte to read: every CRC is the seed
        return torch.full((B,), seed, dtype=torch.int64, device=x.device)
    lib = _lib.load()
    out = torch.empty((B,), dtype=torch.int32, device=x.device)  # the uint32 values' bits
    ws, wsp, wsn = _ws(lib.srx_crc32_scratch_bytes(B, n))
    _lib.check(lib.srx_crc32(_p(x), B, n, n, None if lengths is None else _p(lengths), seed, _p(out), wsp, wsn, _stream()), "srx_crc32")
    return out.to(torch.int64) & 0xFFFFFFFF


def u8_to_float(img_u8, precision=None):
    """uint8 frame -> float on the device (load_gray's cast, run_sr.py:73-75)."""
    prec = precision or get_precision()
    t, _ = _to_dev(img_u8, torch.uint8, as_is=None)  # (any other dtype is cast without a word)
    out = torch.empty(t.shape, dtype=_TORCH_DT[prec], device=t.device)
    _lib.check(_fn("srx_u8_to", prec)(_p(t), t.numel(), _p(out), _stream()), "srx_u8_to")
    return out


def make_gaussian_psf(size=7, sigma=1.0):
    """Normalised 2-D Gaussian PSF (run_sr.py:104-111); host-side, float64."""
    hw = size // 2
    y, x = np.mgrid[-hw:hw + 1, -hw:hw + 1].astype(np.float64)
    k = np.exp(-(x ** 2 + y ** 2) / (2 * sigma ** 2))
    return k / k.sum()


def interleave4(frames_u8):
    """The vendor live view's 4-frame pixel interleave (XPR_Software.py:388-410): uint8 [4, h, w] (or [B, 4, h, w])
    -> uint8 [2h, 2w]; frame k lands on the HR lattice phase its half-pixel shift corresponds to."""
    t, was_np = _to_dev(frames_u8, torch.uint8, as_is=None)  # (as u8_to_float)
    t, single = _batch(t, 4)
    B, four, h, w = t.shape
    if four != 4:
        raise ValueError("interleave4 needs exactly 4 frames")
    out = torch.empty((B, 2 * h, 2 * w), dtype=torch.uint8, device=t.device)
    _lib.check(_lib.load().srx_interleave4_u8(_p(t), B, h, w, _p(out), _stream()), "srx_interleave4_u8")
    return _unbatch(out, single, was_np)


# ------------------------------------------------------------------------------------------
# colour from raw RGGB frames (include/srx_bayer.h): plane p = 0..3 is R, G1, G2, B = raw[p >> 1::2, p & 1::2]
# ------------------------------------------------------------------------------------------
_RAW = (torch.uint8, torch.float32, torch.float64)
_SUFFIX = {torch.uint8: "u8", torch.float32: "f32", torch.float64: "f64"}


def bayer_split(raw):
    """The four Bayer planes of raw frames in one pass (srx_bayer_split_*): [H, W] or [B, H, W], uint8 / float32 / float64 ->
    [4, H/2, W/2] or [B, 4, H/2, W/2] of the same dtype; plane p has the bits of decimate(raw, 2, p >> 1, p & 1).  H and W must be even.
    numpy in -> numpy out."""
    if np.ndim(raw) not in (2, 3):
        raise ValueError("raw must be [H, W] or [B, H, W]")
    x, was_np = _to_dev(raw, what="raw", allowed=_RAW, as_is=None)
    x, single = _batch(x, 3)
    B, H, W = (int(v) for v in x.shape)
    if H % 2 or W % 2:
        raise ValueError(f"bayer_split needs an even H and W (the four planes would differ in size), not {H} x {W}")
    out = torch.empty((B, 4, H // 2, W // 2), dtype=x.dtype, device=x.device)
    name = "srx_bayer_split_" + _SUFFIX[x.dtype]
    _lib.check(getattr(_lib.load(), name)(_p(x), B, H, W, _p(out), _stream()), name)
    return _unbatch(out, single, was_np)


def bayer_mean_u8(stack_u8, precision=None):
    """The mean over R raw uint8 frames, all four Bayer planes from one read of the stack (srx_bayer_mean_u8): uint8 [B, R, H, W] ->
    device tensor [B, 4, H/2, W/2] of the compute precision; plane p has the bits of mean_u8(stack_u8, 2, p >> 1, p & 1)."""
    prec = precision or get_precision()
    B, R, H, W = _shape4(stack_u8, "stack_u8")
    if H % 2 or W % 2:
        raise ValueError(f"bayer_mean_u8 needs an even H and W (the four planes would differ in size), not {H} x {W}")
    x, _ = _to_dev(stack_u8, what="stack_u8", **_BYTES)
    out = torch.empty((B, 4, H // 2, W // 2), dtype=_TORCH_DT[prec], device=x.device)
    _lib.check(_lib.load().srx_bayer_mean_u8(_p(x), B, R, H, W, _ELEM[prec], _p(out), _stream()), "srx_bayer_mean_u8")
    return out


def bayer_merge(planes, factor, gains=None, rgb8=False):
    """Four reconstructed Bayer planes laid over each other as one RGB image (srx_bayer_merge_*): [4, Hp, Wp] or [B, 4, Hp, Wp] ->
    planar [B, 3, Hp, Wp] of the working precision, or with rgb8 the quantised interleaved bytes [B, Hp, Wp, 3].  `factor` is the
    reconstruction's: G1, G2 and B sit one raw pixel = factor / 2 HR samples to the right of / below R, and are read there (clamped at the
    edge); G is the mean of G1 and G2.  factor=0 stacks the planes as they are.  An odd factor would need a half-sample shift of three
    planes and is refused.  gains: three factors (R, G, B), each channel multiplied once; None: none.  numpy in -> numpy out."""
    factor = int(factor)
    if factor < 0 or factor % 2:
        raise ValueError(f"bayer_merge needs an even factor (or 0 to stack the planes): at factor {factor} the planes are offset by "
                         f"{factor / 2} HR samples, and a half-sample shift is an interpolation this call does not make")
    prec = get_precision()
    x, was_np = _to_dev(planes, prec)
    x, single = _batch(x, 4)
    if x.dim() != 4 or x.shape[1] != 4:
        raise ValueError("planes must be [4, Hp, Wp] or [B, 4, Hp, Wp]")
    B, _, Hp, Wp = (int(v) for v in x.shape)
    g = None if gains is None else _host_f64(gains, (3,))
    out = (torch.empty((B, Hp, Wp, 3), dtype=torch.uint8, device=x.device) if rgb8
           else torch.empty((B, 3, Hp, Wp), dtype=x.dtype, device=x.device))
    name = ("srx_bayer_merge_rgb8" if rgb8 else "srx_bayer_merge")
    _lib.check(_fn(name, prec)(_p(x), B, Hp, Wp, factor // 2, None if g is None else g[1], _p(out), _stream()), name)
    out = out[0] if single else out
    return (out.cpu().numpy() if rgb8 else _out(out, True)) if was_np else out


def png_file_rgb8(images):
    """The 8-bit truecolour PNG files of RGB byte images (srx_png_file_rgb8), complete on the device: uint8 [B, H, W, 3] or [H, W, 3] ->
    (files uint8 [B, srx_png_file_rgb8_bound(H, W)], lengths int64 [B]) on the device, nothing synchronised, as png_file.  The IDAT is
    png_deflate's stream of the images viewed as [B, H, 3 W]."""
    if np.ndim(images) not in (3, 4):
        raise ValueError("images must have the shape [B, H, W, 3] or [H, W, 3]")
    x, _ = _batch(_to_dev(images, what="images", **_BYTES)[0], 4)
    B, H, W, C = (int(v) for v in x.shape)
    if C != 3:
        raise ValueError("images must have three interleaved channels")
    lib = _lib.load()
    files = torch.empty((B, lib.srx_png_file_rgb8_bound(H, W)), dtype=torch.uint8, device=x.device)
    lengths = torch.empty((B,), dtype=torch.int64, device=x.device)
    ws, wsp, wsn = _ws(lib.srx_png_file_rgb8_scratch_bytes(B, H, W))
    _lib.check(lib.srx_png_file_rgb8(_p(x), B, H, W, _p(files), _p(lengths), wsp, wsn, _stream()), "srx_png_file_rgb8")
    return files, lengths
