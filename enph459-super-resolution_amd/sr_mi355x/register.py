"""Sub-pixel frame registration on the device (translation only), on top of libsrx.so's `srx_register_*` and, for uint8 frames,
`srx_register_u8_*` (include/srx.h).

Every reconstruction needs the frames' shifts_yx; estimate_shifts measures them from the frames themselves: an integer NCC search
around the caller's table, then Gauss-Newton on the cubic B-spline interpolant of each frame, all on the device with one
device-to-host copy at the end.  The result is in the convention of shifts_yx and goes straight into shift_and_add / ibp.
"""
import numpy as np
import torch

from . import _lib, api

MAX_SEARCH, MIN_CROP = 4, 16
STATUS = {0: "ok", 1: "singular", 2: "search boundary", 3: "not converged"}


def _shape(frames):
    if isinstance(frames, (torch.Tensor, np.ndarray)):
        return tuple(frames.shape)
    if len(frames) == 0:
        raise ValueError("frames is empty")
    return (len(frames),) + tuple(np.shape(frames[0]))


def _check(shape, ref, init, anchor, search, border, n_iter, tol):
    """argument errors, raised before any device work -> (B, N, H, W, batched, init [N, 2] or None, anchor [2])"""
    if len(shape) not in (3, 4):
        raise ValueError(f"frames must be [N, H, W] or [B, N, H, W], got shape {shape}")
    batched = len(shape) == 4
    B, N, H, W = shape if batched else (1,) + shape
    if B < 1 or N < 2:
        raise ValueError(f"need at least one item of two frames, got B={B}, N={N}")
    if N > 32:
        raise ValueError(f"at most 32 frames per item, got {N}")
    if not 0 <= int(ref) < N:
        raise ValueError(f"ref {ref} outside [0, {N})")
    if not 0 <= int(search) <= MAX_SEARCH:
        raise ValueError(f"search {search} outside [0, {MAX_SEARCH}]")
    if int(border) < 0 or int(n_iter) < 0 or not float(tol) >= 0.0:
        raise ValueError(f"border {border}, n_iter {n_iter} and tol {tol} must be >= 0")
    m = int(border) + int(search) + 2
    if H - 2 * m < MIN_CROP or W - 2 * m < MIN_CROP:
        raise ValueError(f"a {H} x {W} frame minus a {m}-pixel margin (border + search + 2) leaves less than {MIN_CROP} x {MIN_CROP}")
    if init is not None:
        init = np.ascontiguousarray(np.asarray(init, dtype=np.float64))
        if init.shape != (N, 2) or not np.all(np.isfinite(init)):
            raise ValueError(f"init must be a finite [{N}, 2] table, got shape {init.shape}")
    if anchor is None:
        anchor = init[int(ref)] if init is not None else np.zeros(2)
    anchor = np.asarray(anchor, dtype=np.float64)
    if anchor.shape != (2,) or not np.all(np.isfinite(anchor)):
        raise ValueError(f"anchor must be a finite (dy, dx), got {anchor!r}")
    return B, N, H, W, batched, init, anchor


def workspace_bytes(elem_bytes, B, N, H, W, search):
    """srx_register_workspace_bytes (no GPU needed)"""
    return int(_lib.load().srx_register_workspace_bytes(int(elem_bytes), int(B), int(N), int(H), int(W), int(search)))


def estimate_shifts(frames, ref=0, init=None, anchor=None, search=2, border=8, n_iter=10, tol=1e-4, precision=None, full=False):
    """Shifts of the frames, in LR pixels (dy, dx) in the convention of shifts_yx, estimated on the device.

    frames: a list or stack of [H, W] frames, or a [B, N, H, W] tensor (one registration per item).  init: the [N, 2] shift table
    the frames were taken with (the coarse search starts at rint(init[k] - init[ref])); anchor: the reference frame's known shift
    (default init[ref], or (0, 0)).  Returns host float64 anchor + d_k, [N, 2] (or [B, N, 2]); with full=True also the zero-mean
    NCC score at the returned shift and the status per frame (0 ok, 1 singular, 2 coarse argmax on the search boundary, 3 not
    converged; see STATUS), float64 and int32 [N] (or [B, N]).  Frames with a nonzero status are best replaced by the table.
    uint8 frames (the camera's own samples) are uploaded and registered as bytes (srx_register_u8_*): the same bits as the frames
    converted to the compute precision give, with no float copy of them anywhere."""
    B, N, H, W, batched, init, anchor = _check(_shape(frames), ref, init, anchor, search, border, n_iter, tol)
    prec = precision or api.get_precision()
    name = "srx_register_u8" if api._is_u8(frames) else "srx_register"  # (uint8 frames go up and stay as they are)
    x = api._stack_dev(frames, None if name == "srx_register_u8" else prec)[0].reshape(B, N, H, W)
    dev = x.device
    shifts = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    score = torch.empty((B, N), dtype=torch.float64, device=dev)
    status = torch.empty((B, N), dtype=torch.int32, device=dev)
    wt, wp, wn = api._ws(workspace_bytes(api._ELEM[prec], B, N, H, W, search))
    hinit = None if init is None else init.ctypes.data_as(_lib._HD)
    _lib.check(api._fn(name, prec)(api._p(x), B, N, H, W, int(ref), hinit, int(search), int(border), int(n_iter), float(tol),
                                   api._p(shifts), api._p(score), api._p(status), wp, wn, api._stream()), name)
    d = shifts.cpu().numpy() + anchor
    sc, st = score.cpu().numpy(), status.cpu().numpy()
    if not batched:
        d, sc, st = d[0], sc[0], st[0]
    return (d, sc, st) if full else d
