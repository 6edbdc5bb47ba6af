"""Patch-wise reconstruction with locally registered shifts, on top of libsrx.so's `srx_patches_gather_*` / `srx_patches_blend_*`
(include/srx.h) and the batched per-item calls.

A tilting-plate pixel shifter in a non-telecentric beam does not shift the whole field equally, and the reference reconstructs a
session under one shift table.  Here a frame stack is cut into overlapping patches (gather), every patch is registered on its own
(estimate_shifts with B = patches: the shift FIELD, itself a calibration result), the patches are reconstructed as one batch in
which every item has its own table (shift_and_add_batched / ibp_batched with [P, N, 2] tables), and the HR patches are blended back
into one image (blend).  Opt-in: nothing else in the package calls this unless asked (session.reconstruct(patchwise=...)).

Grid rule per axis (n samples, patch length L, stride s): count = ceil((n - L) / s) + 1, origin(i) = min(i s, n - L) -- the last
patch is pulled inward, never padded.  The HR grid is the LR grid times the factor, so patch p of the LR frames reconstructs to
patch p of the HR image.
"""
import numpy as np
import torch

from . import _lib, api

STATUS_REJECTED = 4  # estimate further than max_dev from the table: the table shift is kept (0..3: register.STATUS)


class PatchGrid:
    """The patches of an h x w LR frame (and of its factor-times larger reconstruction): square patches of `patch_lr` LR samples that
    overlap their neighbours by `overlap_lr`; the blend gives no weight to the outer `margin_hr` HR samples of a patch (image edges
    excepted) and ramps over the rest of the overlap.
      gy, gx, P              patches per axis and in all; patch p = iy gx + ix
      oy_lr, ox_lr           origins [gy], [gx] in LR samples; oy_hr, ox_hr the same in HR samples
      L_hr, s_hr             patch length and stride in HR samples: factor patch_lr, factor (patch_lr - overlap_lr)
      centres_lr, centres_hr [gy, gx, 2] (y, x) of the patch centres, in samples of the LR frame / the HR image"""

    def __init__(self, h, w, factor, patch_lr=None, overlap_lr=16, margin_hr=8):
        self.h, self.w, self.factor = int(h), int(w), int(factor)
        self.patch_lr = 256 // self.factor if patch_lr is None else int(patch_lr)
        self.overlap_lr, self.margin_hr = int(overlap_lr), int(margin_hr)
        self.s_lr = self.patch_lr - self.overlap_lr
        self.L_hr, self.s_hr = self.factor * self.patch_lr, self.factor * self.s_lr
        self.H, self.W = self.h * self.factor, self.w * self.factor
        lib = _lib.load()
        self.gy, self.gx = lib.srx_patches_count(self.h, self.patch_lr, self.s_lr), lib.srx_patches_count(self.w, self.patch_lr, self.s_lr)
        if self.factor < 1 or self.gy == 0 or self.gx == 0:
            raise ValueError(f"no patch grid for a {h} x {w} frame with patch_lr={self.patch_lr}, overlap_lr={self.overlap_lr}: the patch must fit "
                             "the frame and the stride patch_lr - overlap_lr must lie in [patch_lr / 2, patch_lr]")
        if self.margin_hr < 0 or self.L_hr - self.s_hr - 2 * self.margin_hr < 1:
            raise ValueError(f"margin_hr={self.margin_hr} leaves no ramp in an overlap of {self.L_hr - self.s_hr} HR samples")
        self.P = self.gy * self.gx
        self.oy_lr = np.minimum(np.arange(self.gy) * self.s_lr, self.h - self.patch_lr)
        self.ox_lr = np.minimum(np.arange(self.gx) * self.s_lr, self.w - self.patch_lr)
        self.oy_hr, self.ox_hr = self.oy_lr * self.factor, self.ox_lr * self.factor
        oy, ox = np.meshgrid(self.oy_lr, self.ox_lr, indexing="ij")
        self.centres_lr = np.stack([oy, ox], axis=-1) + (self.patch_lr - 1) / 2.0
        self.centres_hr = self.factor * np.stack([oy, ox], axis=-1) + (self.L_hr - 1) / 2.0

    def describe(self):
        """the grid as plain lists (shift_field.json)"""
        return {"h": self.h, "w": self.w, "factor": self.factor, "patch_lr": self.patch_lr, "overlap_lr": self.overlap_lr,
                "margin_hr": self.margin_hr, "gy": self.gy, "gx": self.gx, "origins_lr_y": self.oy_lr.tolist(),
                "origins_lr_x": self.ox_lr.tolist(), "centres_lr_yx": self.centres_lr.tolist(), "centres_hr_yx": self.centres_hr.tolist()}


_GATHER = {torch.uint8: "srx_patches_gather_u8", torch.float32: "srx_patches_gather_f32", torch.float64: "srx_patches_gather_f64"}
_BLEND = {torch.float32: "srx_patches_blend_f32", torch.float64: "srx_patches_blend_f64"}


_AS_IS = (np.uint8, np.float32, np.float64)  # host arrays of these element types are kept; any other becomes float64 (api._to_dev)


def gather(frames, grid):
    """frames [N, h, w] or [B, N, h, w] (uint8, float32 or float64; the element type is kept) -> device tensor [B P, N, patch_lr,
    patch_lr], the layout of the batched per-item calls: item b P + iy gx + ix is the patch at (grid.oy_lr[iy], grid.ox_lr[ix]) of
    batch item b (srx_patches_gather_*: one launch, a pure index map)."""
    x, _ = api._batch(api._to_dev(frames, allowed=_GATHER, as_is=_AS_IS, what="frames")[0], 4)
    if x.dim() != 4 or tuple(x.shape[2:]) != (grid.h, grid.w):
        raise ValueError(f"frames must be [N, {grid.h}, {grid.w}] or [B, N, {grid.h}, {grid.w}], not {tuple(x.shape)}")
    B, N = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((B * grid.P, N, grid.patch_lr, grid.patch_lr), dtype=x.dtype, device=x.device)
    name = _GATHER[x.dtype]
    _lib.check(getattr(_lib.load(), name)(api._p(x), B, N, grid.h, grid.w, grid.patch_lr, grid.patch_lr, grid.s_lr, grid.s_lr, api._p(out),
                                          api._stream()), name)
    return out


def blend(hr_patches, grid):
    """HR patches [B P, L_hr, L_hr] (float32 or float64) -> device tensor [B, H, W]: every sample the weighted mean of the patches
    over it, weights as include/srx.h states them (srx_patches_blend_*: one launch)."""
    x, _ = api._to_dev(hr_patches, allowed=_BLEND, as_is=_AS_IS, what="hr_patches")
    if x.dim() != 3 or tuple(x.shape[1:]) != (grid.L_hr, grid.L_hr) or x.shape[0] % grid.P or x.shape[0] == 0:
        raise ValueError(f"hr_patches must be [B * {grid.P}, {grid.L_hr}, {grid.L_hr}], not {tuple(x.shape)}")
    B = int(x.shape[0]) // grid.P
    out = torch.empty((B, grid.H, grid.W), dtype=x.dtype, device=x.device)
    name = _BLEND[x.dtype]
    _lib.check(getattr(_lib.load(), name)(api._p(x), B, grid.H, grid.W, grid.L_hr, grid.L_hr, grid.s_hr, grid.s_hr, grid.margin_hr,
                                          api._p(out), api._stream()), name)
    return out


def estimate_shift_field(frames, init, grid, max_dev=0.5, ref=0, **kwargs):
    """The frames' shifts per patch: frames [N, h, w] are gathered and registered in ONE estimate_shifts call with B = P items,
    init = the table the frames were taken with and anchor = init[ref]; kwargs go to estimate_shifts (search, border, n_iter, tol,
    precision).  -> dict of host arrays shaped [gy, gx, N, ...]: `estimated` [.., 2], `used` [.., 2], `score`, `status`.  A frame of a
    patch keeps the TABLE shift where its status is nonzero (as session.register_shifts does) and where the estimate departs from the
    table by more than max_dev LR pixels on either axis; the latter is recorded as status 4, "rejected"."""
    if not isinstance(frames, (torch.Tensor, np.ndarray)):
        frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack(frames)
    if len(frames.shape) != 3:
        raise ValueError("estimate_shift_field takes the [N, h, w] frames of one image")
    return _field_of_patches(gather(frames, grid), init, grid, max_dev, ref, **kwargs)


def _field_of_patches(patches, init, grid, max_dev=0.5, ref=0, **kwargs):
    """estimate_shift_field on the gathered patches [P, N, patch_lr, patch_lr]"""
    from . import register
    table = np.ascontiguousarray(np.asarray(init, dtype=np.float64))
    N = int(patches.shape[1])
    if table.shape != (N, 2):
        raise ValueError(f"init must be the [{N}, 2] shift table of the frames")
    est, score, status = register.estimate_shifts(patches, ref=ref, init=table, anchor=table[int(ref)], full=True, **kwargs)
    status = status.astype(np.int32)
    far = (np.abs(est - table[None]).max(axis=-1) > float(max_dev)) & (status == 0)
    status[far] = STATUS_REJECTED
    used = np.where((status == 0)[..., None], est, table[None])
    shp = (grid.gy, grid.gx, N)
    return {"estimated": est.reshape(shp + (2,)), "used": used.reshape(shp + (2,)), "score": score.reshape(shp), "status": status.reshape(shp)}


def field_json(grid, table, field):
    """shift_field.json: the grid, the patch centres and the field, as plain lists"""
    return {"grid": grid.describe(), "nominal": np.asarray(table, dtype=np.float64).tolist(),
            **{k: np.asarray(field[k]).tolist() for k in ("estimated", "used", "score", "status")}}


def reconstruct_patchwise(frames, shifts, psf_kernel, n_iter, factor=2, step=0.5, grid=None, local=True, max_dev=0.5):
    """session.reconstruct patch by patch: gather -> (local) shift field -> shift_and_add[_u8]_batched -> ibp[_u8]_batched with the
    [P, N, 2] tables -> blend of the SAA patches and of the IBP patches.
    frames: a list of [h, w] device frames, float or uint8 (uint8 frames go through as bytes: the same bits); grid: a PatchGrid
    (default PatchGrid(h, w, factor)).  -> (images, trace, field): the image dict of session.reconstruct ("native_2x" and "LR_mean"
    stay whole-frame, exactly as there; "SAA" and "SAA_IBP" are blended), the MSE trace and the field of estimate_shift_field (None
    with local=False).
    The trace is the equal-weight mean over the patches of the per-item traces.  That is NOT the whole image's trace: overlaps count
    twice, and the clamped last row and column of patches overlap more than the others.
    local=False runs every patch under the one table `shifts`, as a single shared-table batch: the baseline against which the
    field's deviation and gain are measured.
    Routes are whatever the library's router gives and are not changed here: at x2 in float32 per-patch tables go to "btile" as one
    batch; in float64, or at x3 / x4, items with pairwise different tables run one by one on "fused" -- slow, but correct."""
    from . import session
    lr = torch.stack(list(frames)) if not isinstance(frames, torch.Tensor) else frames
    if lr.dim() != 3:
        raise ValueError("frames must be N frames of one [h, w] image")
    N, h, w = (int(v) for v in lr.shape)
    grid = PatchGrid(h, w, factor) if grid is None else grid
    if (grid.h, grid.w, grid.factor) != (h, w, int(factor)):
        raise ValueError("grid does not belong to these frames and this factor")
    table = np.ascontiguousarray(np.asarray(shifts, dtype=np.float64))
    u8 = lr.dtype == torch.uint8
    mean_lr = session._frame_mean(lr[None])[0]
    native = api.zoom_batched(mean_lr[None], factor)[0]
    patches = gather(lr if u8 else lr.to(api._TORCH_DT[api.get_precision()]), grid)
    field, tables = None, table
    if local:
        field = _field_of_patches(patches, table, grid, max_dev=max_dev)
        tables = np.ascontiguousarray(field["used"].reshape(grid.P, N, 2))
    saa_fn, ibp_fn = (api.shift_and_add_u8_batched, api.ibp_u8_batched) if u8 else (api.shift_and_add_batched, api.ibp_batched)
    saa = saa_fn(patches, tables, factor)
    hr, errs = ibp_fn(patches, tables, psf_kernel, saa.clone(), factor, n_iter, step)
    images = {"native_2x": native, "SAA": blend(saa, grid)[0], "SAA_IBP": blend(hr, grid)[0], "LR_mean": mean_lr}
    return images, [float(e) for e in errs.mean(dim=0).cpu()], field
