"""The measured PSF from pinhole frames on the device, on top of libsrx.so's `srx_psf_estimate_*` (include/srx.h).

The device form of session.psf_from_pinhole_images (load_measured_psf, mono_cal_target/run_sr.py:114-152): the arg-max of every
frame, the +-(halfwidth + 6) window around it, the windows' mean, the central cut, background off, clip, sum 1 -- three kernel
launches and one device-to-host copy of the (2 halfwidth + 1)^2 result, which goes straight into ibp as `kernel=`.  uint8 frames
(what the camera and the PNGs hold) are read as they are; float frames in the working precision.
"""
import numpy as np
import torch

from . import _lib, api, session

MAX_HALFWIDTH, EXTRA_REACH = 7, 6
CHUNK_BYTES = 32768  # of one frame per workgroup of the arg-max kernel (csrc/srx_psf.hpp)


def _check(frames, halfwidth):
    """argument errors, raised before any device work -> (N, H, W, is_u8)"""
    hw = int(halfwidth)
    if hw != halfwidth or not 1 <= hw <= MAX_HALFWIDTH:
        raise ValueError(f"halfwidth {halfwidth} outside [1, {MAX_HALFWIDTH}]")
    if isinstance(frames, (torch.Tensor, np.ndarray)):
        shape = tuple(frames.shape)
        if len(shape) != 3:
            raise ValueError(f"frames must be [N, H, W], got shape {shape}")
    else:
        frames = list(frames)
        if len(frames) == 0:
            raise ValueError("frames is empty")
        shapes = {tuple(np.shape(f)) for f in frames}
        if len(shapes) != 1:
            raise ValueError(f"frames of mixed shape: {sorted(shapes)}")
        (hw_shape,) = shapes
        if len(hw_shape) != 2:
            raise ValueError(f"every frame must be [H, W], got shape {hw_shape}")
        shape = (len(frames),) + hw_shape
    N, H, W = shape
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"frames is empty: shape {shape}")
    if N > 65535:
        raise ValueError(f"at most 65535 frames, got {N}")
    return N, H, W, api._is_u8(frames)


def workspace_bytes(elem_bytes, N, H, W, halfwidth=session.PSF_HALFWIDTH):
    """srx_psf_estimate_workspace_bytes (no GPU needed)"""
    return int(_lib.load().srx_psf_estimate_workspace_bytes(int(elem_bytes), int(N), int(H), int(W), int(halfwidth)))


def estimate_psf(frames, halfwidth=session.PSF_HALFWIDTH, full=False, precision=None):
    """The normalised (2 halfwidth + 1)^2 PSF of a list or stack of [H, W] pinhole frames (numpy uint8 / float, or device tensors),
    host float64, ready to pass as `kernel=` to ibp.  full=True: also the peaks, int32 [N, 2] (row, column; reported for dropped
    frames too) and used, bool [N] (the frame's window lay inside it).  FileNotFoundError("no usable pinhole image") when no frame
    is used, as session.psf_from_pinhole_images."""
    N, H, W, is_u8 = _check(frames, halfwidth)
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = list(frames)
    if is_u8:
        x, fn, eb = api._stack_dev(frames)[0], _lib.load().srx_psf_estimate_u8, 1
    else:
        prec = precision or api.get_precision()
        x, _ = api._stack_dev(frames, prec)
        fn, eb = api._fn("srx_psf_estimate", prec), api._ELEM[prec]
    side = 2 * int(halfwidth) + 1
    psf = torch.empty((side, side), dtype=torch.float64, device=x.device)
    info = torch.empty((N, 3), dtype=torch.int32, device=x.device)
    wt, wp, wn = api._ws(workspace_bytes(eb, N, H, W, halfwidth))
    _lib.check(fn(api._p(x), N, H, W, int(halfwidth), api._p(psf), api._p(info), wp, wn, api._stream()), "srx_psf_estimate")
    out = torch.cat([psf.reshape(-1), info.reshape(-1).to(torch.float64)]).cpu().numpy()  # the one device-to-host copy
    kernel, info_h = out[:side * side].reshape(side, side).copy(), out[side * side:].reshape(N, 3).astype(np.int32)
    if not info_h[:, 2].any():
        raise FileNotFoundError("no usable pinhole image")
    return (kernel, info_h[:, :2].copy(), info_h[:, 2].astype(bool)) if full else kernel
