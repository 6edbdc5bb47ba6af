"""Device forms of the quality metrics on top of libsrx.so's `srx_pair_moments_*`, `srx_local_contrast_*`,
`srx_ring_sums_*`, `srx_spot_moments_*`, `srx_edge_magnitude_f64`, `srx_edge_dist_range`, `srx_edge_bins_*`, `srx_ssim_*` (include/srx.h).

Same names, arguments and return values as `sr_mi355x.metrics` (which mirrors the reference's notebook / calibration functions:
mono_cal_target/analysis.ipynb cells 4, 7, 10; data_collection/psf_mtf_utils.py:67-178; the vendor GUI's affine-fit PSNR,
opt_materials/software/XPR_Software.py:735-745, 1215-1256), but the images stay on the GPU: what runs on the device is every pass over
a frame or an ROI (the 12.6 MP PSNR reductions, the ROI's Gaussian + Sobel, the projection and 1/4-px binning, the ring means, the
sliding-window contrast); what stays on the host are the few-thousand-operation tails -- the 85th percentile and the two line fits of
the edge pixels, the ESF interpolation, the 72-sample gradient / Hann / FFT (metrics.esf_to_mtf), the 7-parameter Gaussian fit and the
256^2 FFT of compute_mtf.  There is no CPU fallback for the device parts: without libsrx.so / a GPU these functions raise.

`edge_sfr` (srx_edge_sfr_*) is the slanted-edge chain whole -- percentile, fits, ESF, MTF50 / MTF10 -- for a batch of ROIs in one call
without a host step; `cal_target_report(fused=True)` and `session.queue_metrics_device` are built on it.
"""
import ctypes

import numpy as np
import torch

from . import _lib, api, metrics

_c = ctypes


def _image(x, prec=None):
    """-> (contiguous CUDA tensor, 'f32' | 'f64'): float32 tensors are computed in float32, everything else (uint8 / float alike: the
    notebook works on the PNGs' values as float64) in float64, unless `prec` says which; host arrays go up as float64 (api._to_dev)"""
    prec = prec or ("f32" if isinstance(x, torch.Tensor) and x.dtype == torch.float32 else "f64")
    return api._to_dev(x, prec, as_is=())[0], prec


def _ws(B, H, W, nbin):
    return api._ws(_lib.load().srx_metrics_workspace_bytes(int(B), int(H), int(W), int(nbin)))


def pair_moments(ref, test, border=0):
    """[B, 7] float64 (host): n, sum t, sum r, sum t^2, sum t r, sum r^2, sum (r - t)^2 over ref / test [B, H, W] (or [H, W]) minus a
    `border`-pixel frame, one fused pass over the two device images."""
    return pair_moments_device(ref, test, border).cpu().numpy()


def pair_moments_device(ref, test, border=0):
    """pair_moments without the copy back: the [B, 7] float64 device tensor, nothing synchronised"""
    r, t, prec, _ = _pair(ref, test)
    B, H, W = r.shape
    out = torch.empty((B, 7), dtype=torch.float64, device=r.device)
    wt, wp, wn = _ws(B, H, W, 1)
    _lib.check(api._fn("srx_pair_moments", prec)(api._p(r), api._p(t), B, H, W, int(border), api._p(out), wp, wn, api._stream()), "srx_pair_moments")
    return out


def psnr_from_moments(row, peak=255.0):
    """psnr's value from one row of pair_moments"""
    return float("inf") if row[6] == 0.0 else float(10.0 * np.log10(peak * peak * row[0] / row[6]))


def psnr_affine_from_moments(row, data_range=1.0):
    """psnr_affine's value from one row of pair_moments (taken with its border)"""
    n, st, sr, stt, strr, srr, _ = row
    s_tt, s_tr, s_rr = stt - st * st / n, strr - st * sr / n, srr - sr * sr / n
    mse = max((s_rr - (s_tr * s_tr / s_tt if s_tt > 0 else 0.0)) / n, 0.0) / (255.0 * 255.0)
    return np.inf if mse == 0 else 10.0 * np.log10(data_range ** 2 / mse)


def psnr(a, b, peak=255.0):
    """10 log10(peak^2 / MSE) of two device images, per item for a batch; float (or a list for a batch)."""
    v = [psnr_from_moments(row, peak) for row in pair_moments(a, b)]
    return v[0] if len(v) == 1 else v


def psnr_affine(ref, test, border=10, data_range=1.0):
    """metrics.psnr_affine on device images: the least-squares line test -> a test + b from the five second-order moments, then
    MSE = (S_rr - S_tr^2 / S_tt) / n in centred moments, everything scaled to [0, 1] from 8-bit."""
    return psnr_affine_from_moments(pair_moments(ref, test, border=border)[0], data_range)


def _np_dtype(x):
    """numpy dtype of a tensor / array (what decides SSIM's default data_range)"""
    return np.dtype(str(x.dtype).replace("torch.", "")) if isinstance(x, torch.Tensor) else np.asarray(x).dtype


def _pair(ref, test):
    """-> (ref, test) as [B, H, W] device tensors of one precision, the precision, whether the input was one image"""
    r, prec = _image(ref)
    t, _ = _image(test, prec)
    r, one = api._batch(r, 3)
    if one:
        t = t[None]
    if r.shape != t.shape or r.dim() != 3:
        raise ValueError("ref and test must be [H, W] or [B, H, W] of the same shape")
    return r, t, prec, one


def _ssim(r, t, prec, one, dtype, affine, *, win_size=None, data_range=None, gaussian_weights=False, sigma=1.5, use_sample_covariance=True,
          K1=0.01, K2=0.03, full=False, border=0):
    B, H, W = r.shape
    h, w = H - 2 * border, W - 2 * border
    if border < 0 or h <= 0 or w <= 0:
        raise ValueError(f"border {border} leaves nothing of a {H} x {W} image")
    rad, taps, dr = metrics.ssim_params((h, w), dtype, win_size, data_range, gaussian_weights, sigma)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    mssim = torch.empty(B, dtype=torch.float64, device=r.device)
    smap = torch.empty((B, h, w), dtype=r.dtype, device=r.device) if full else None
    aff = None if affine is None else _image(affine, "f64")[0]
    wt, wp, wn = _ws(B, H, W, 1)
    _lib.check(api._fn("srx_ssim", prec)(api._p(r), api._p(t), B, H, W, int(border), rad, taps.ctypes.data_as(_lib._HD),
                                         int(bool(use_sample_covariance)), dr, float(K1), float(K2), None if aff is None else api._p(aff),
                                         api._p(mssim), None if smap is None else api._p(smap), wp, wn, api._stream()), "srx_ssim")
    m = [float(v) for v in mssim.cpu().numpy()]
    m = m[0] if one else m
    if not full:
        return m
    return m, (smap[0] if one else smap)


def ssim(ref, test, *, win_size=None, data_range=None, gaussian_weights=False, sigma=1.5, use_sample_covariance=True, K1=0.01, K2=0.03,
         full=False, border=0):
    """metrics.ssim (skimage structural_similarity, 2-D) of device images [H, W] or [B, H, W] in one pass over the pair (srx_ssim):
    a float, or a list for a batch; with full=True also the map S over the crop as a device tensor ([h, w] or [B, h, w]).  float32
    tensors are computed in float32, everything else in float64; data_range defaults to the input dtype's integer range."""
    r, t, prec, one = _pair(ref, test)
    return _ssim(r, t, prec, one, _np_dtype(ref), None, win_size=win_size, data_range=data_range, gaussian_weights=gaussian_weights,
                 sigma=sigma, use_sample_covariance=use_sample_covariance, K1=K1, K2=K2, full=full, border=border)


def ssim_affine(ref, test, border=10, data_range=1.0, **kw):
    """metrics.ssim_affine on device images (per item for a batch): the line test -> a test + b from the pair's moments (as
    psnr_affine), then SSIM of ref / 255 against (a / 255) test + b / 255 with the affine applied inside the kernel (no fitted
    copy).  Parity with the vendor GUI is unpinned, as for metrics.ssim_affine."""
    r, t, prec, one = _pair(ref, test)
    aff = []
    for n, st, sr, stt, strr, _, _ in pair_moments(r, t, border=border):
        s_tt, s_tr = stt - st * st / n, strr - st * sr / n
        a = s_tr / s_tt if s_tt > 0 else 0.0
        aff.append((1.0 / 255.0, a / 255.0, (sr - a * st) / n / 255.0))
    return _ssim(r, t, prec, one, np.float64, np.asarray(aff), data_range=data_range, border=border, **kw)


def ecc(ref, test, border=0):
    """metrics.ecc of device images (a float, or a list for a batch): the zero-mean normalised cross-correlation from the pair's
    moments (srx_pair_moments); nan when either crop is constant.  Parity with cv2.computeECC is unpinned."""
    v = []
    for n, st, sr, stt, strr, srr, _ in pair_moments(ref, test, border=border):
        s_tt, s_tr, s_rr = stt - st * st / n, strr - st * sr / n, srr - sr * sr / n
        den = np.sqrt(s_tt * s_rr) if s_tt > 0 and s_rr > 0 else 0.0
        v.append(float(s_tr / den) if den > 0 else float("nan"))
    return v[0] if len(v) == 1 else v


def local_contrast(profile, window=20):
    """metrics.local_contrast of a device profile [n] (or [B, n]); float64 numpy out."""
    p, one = api._batch(_image(profile, "f64")[0], 2)
    return api._unbatch(local_contrast_device(p, window), one, True)


def radial_average(data_2d, center=None, max_radius=None):
    """metrics.radial_average on a device image: (radii, ring means)."""
    d, prec = _image(data_2d)
    h, w = d.shape
    cy, cx = (0.5 * h, 0.5 * w) if center is None else center
    if max_radius is None:
        max_radius = int(min(cy, cx, h - cy, w - cx))
    nbin = max(int(max_radius), 0)
    if nbin == 0:
        return np.arange(0), np.zeros(0)
    out = torch.empty(2 * nbin, dtype=torch.float64, device=d.device)
    wt, wp, wn = _ws(1, h, w, nbin)
    _lib.check(api._fn("srx_ring_sums", prec)(api._p(d), h, w, float(cy), float(cx), nbin, api._p(out), wp, wn, api._stream()), "srx_ring_sums")
    o = out.cpu().numpy()
    tot, cnt = o[:nbin], o[nbin:]
    return np.arange(nbin), np.divide(tot, cnt, out=np.zeros(nbin), where=cnt > 0)


def subpixel_centre(psf):
    """metrics.subpixel_centre on a device PSF image: (row, col) first moments where it exceeds a tenth of its peak."""
    p, prec = _image(psf)
    out = torch.empty(4, dtype=torch.float64, device=p.device)
    _lib.check(api._fn("srx_spot_moments", prec)(api._p(p), p.shape[0], p.shape[1], api._p(out), api._stream()), "srx_spot_moments")
    _, mass, sy, sx = out.cpu().numpy()
    return float(sy / mass), float(sx / mass)


def compute_mtf(psf, pixel_pitch_um=None):
    """metrics.compute_mtf with the ring means of the 2-D MTF taken on the device (the 256^2 FFT stays on the host)."""
    psf = np.asarray(psf.cpu().numpy() if isinstance(psf, torch.Tensor) else psf, dtype=np.float64)
    _, _, mtf_2d, label, nyq = metrics.compute_mtf(psf, pixel_pitch_um)
    n = mtf_2d.shape[0]
    rings, mtf_radial = radial_average(mtf_2d, (0.5 * n, 0.5 * n), n // 2)
    per_px = rings / float(n)
    return (per_px if pixel_pitch_um is None else per_px / (pixel_pitch_um * 1e-3)), mtf_radial, mtf_2d, label, nyq


def edge_magnitude(roi, sigma=1.5):
    """Sobel magnitude of the Gaussian-smoothed ROI (scipy.ndimage 'reflect' boundaries), device float64 tensor."""
    r, _ = _image(roi, "f64")
    h, w = r.shape
    mag = torch.empty_like(r)
    wt, wp, wn = _ws(1, h, w, 1)
    _lib.check(_lib.load().srx_edge_magnitude_f64(api._p(r), h, w, float(sigma), api._p(mag), wp, wn, api._stream()), "srx_edge_magnitude")
    return mag


def slanted_edge_esf(roi, side="left", verbose=False):
    """metrics.slanted_edge_esf with the ROI on the device: the Gaussian + Sobel magnitude, the projection of every pixel on the edge's
    normal and the 1/4-px binning run in libsrx; the percentile and the two line fits over the edge pixels run on the host from the
    magnitude image (one small device-to-host copy).  Returns (esf_x, esf_y, angle_deg)."""
    lib = _lib.load()
    r, _ = _image(roi, "f64")
    h, w = r.shape
    mag = edge_magnitude(r).cpu().numpy()
    rs, cs = np.where(mag > np.percentile(mag, 85))
    if len(rs) < 20:
        raise RuntimeError("Too few edge pixels detected")
    rows_are_x = bool((rs.max() - rs.min()) >= (cs.max() - cs.min()))
    u, v = (rs, cs) if rows_are_x else (cs, rs)
    m_c, b_c = np.polyfit(u, v, 1)
    edge_dist = (v - m_c * u - b_c) / np.sqrt(1 + m_c ** 2)
    sel = edge_dist < 0 if side == "left" else edge_dist > 0
    if sel.sum() < 10:
        raise RuntimeError(f"Too few edge pixels on {side} side")
    m, b = np.polyfit(u[sel], v[sel], 1)
    norm = float(np.sqrt(1 + m ** 2))
    angle = np.degrees(np.arctan2(1, m)) if rows_are_x else np.degrees(np.arctan2(m, 1))
    if verbose:
        print(f"  Edge angle: {angle:.1f} deg, {int(sel.sum())}/{len(rs)} edge pixels ({side} side)")
    rng = torch.empty(2, dtype=torch.float64, device=r.device)
    _lib.check(lib.srx_edge_dist_range(h, w, float(m), float(b), norm, int(rows_are_x), api._p(rng), api._stream()), "srx_edge_dist_range")
    lo, hi = (float(x) for x in rng.cpu().numpy())
    bw = 0.25
    bins = np.arange(lo, hi + bw, bw)  # the edges the device forms as lo + i * bw
    esf_x = 0.5 * (bins[:-1] + bins[1:])
    nbin = len(esf_x)
    out = torch.empty(2 * nbin, dtype=torch.float64, device=r.device)
    wt, wp, wn = _ws(1, h, w, nbin)
    _lib.check(lib.srx_edge_bins_f64(api._p(r), h, w, float(m), float(b), norm, int(rows_are_x), lo, bw, nbin, api._p(out), wp, wn, api._stream()),
               "srx_edge_bins")
    o = out.cpu().numpy()
    tot, cnt = o[:nbin], o[nbin:]
    esf_y = np.full(nbin, np.nan)
    np.divide(tot, cnt, out=esf_y, where=cnt > 0)
    valid = ~np.isnan(esf_y)
    if valid.sum() > 2:
        esf_y = np.interp(esf_x, esf_x[valid], esf_y[valid])
    if esf_y[-1] < esf_y[0]:
        esf_x, esf_y = -esf_x[::-1], esf_y[::-1]
    return esf_x, esf_y, angle


EDGE_MAX_BINS, EDGE_SUMMARY = 80, 16  # SRX_EDGE_MAX_BINS, SRX_EDGE_SUMMARY (include/srx.h)
EDGE_FIELDS = ("mtf50", "mtf10", "angle_deg", "m", "b", "rows_are_x", "threshold", "n_edge", "n_side", "nbin", "lo", "hi", "flipped", "m_c", "b_c")
EDGE_STATUS = {1: "Too few edge pixels detected", 2: "Too few edge pixels on the chosen side", 3: "degenerate edge fit",
               4: "too few non-empty ESF bins"}
_EDGE_KINDS = {torch.uint8: "u8", torch.float32: "f32", torch.float64: "f64"}


class EdgeSfr:
    """The device outputs of one edge_sfr call: `summary` [B, 16], `esf` [B, 2, 80], `mtf` [B, 2, 40] (float64) and `status` [B] (int32), views
    of ONE device block, so that result() is one copy.  Nothing has synchronised when the call returns."""

    def __init__(self, block, B, one, keep):
        self.block, self.B, self.one, self._keep, self._host = block, B, one, keep, None
        self.summary, self.esf, self.mtf, self.status = self._views(block)

    def _views(self, blk):
        B, n, h = self.B, EDGE_SUMMARY, EDGE_MAX_BINS
        return (blk[:B * n].view(B, n), blk[B * n:B * (n + 2 * h)].view(B, 2, h), blk[B * (n + 2 * h):B * (n + 3 * h)].view(B, 2, h // 2),
                blk[B * (n + 3 * h):].view(torch.int32)[:B])

    def start_copy(self):
        """queue the copy into a pinned host buffer (non-blocking); result() then reads that buffer, so wait for an event recorded behind
        this call first"""
        self._host = torch.empty(self.block.shape, dtype=self.block.dtype, pin_memory=True)
        self._host.copy_(self.block, non_blocking=True)
        return self

    def result(self):
        """The one copy back (or the pinned buffer of start_copy) -> per item a dict: mtf50, mtf10 (cycles per ROI pixel, nan where the
        curve never falls through), angle_deg, esf_x, esf_y, freq, mtf, status and the other summary fields; a list for a batch."""
        summary, esf, mtf, status = (t.numpy() for t in self._views(self._host if self._host is not None else self.block.cpu()))
        items = []
        for b in range(self.B):
            d = {k: float(v) for k, v in zip(EDGE_FIELDS, summary[b])}
            st = int(status[b])
            nbin = int(d["nbin"]) if st == 0 else 0
            d.update(status=st, esf_x=esf[b, 0, :nbin].copy(), esf_y=esf[b, 1, :nbin].copy(), freq=mtf[b, 0, :nbin // 2].copy(),
                     mtf=mtf[b, 1, :nbin // 2].copy())
            items.append(d)
        return items[0] if self.one else items


def edge_sfr(images, side="left", sigma=1.5):
    """The slanted-edge SFR of device ROIs in one call (srx_edge_sfr_*): metrics.slanted_edge_esf -> esf_to_mtf -> mtf_at_fraction with no
    host step.  `images`: a CUDA tensor [H, W] or [B, H, W], uint8 / float32 / float64; it may be a ROI view of larger frames as long as
    its columns are adjacent (the row and item strides are passed on, nothing is copied).  Returns an EdgeSfr; nothing synchronises
    before its result()."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda or images.dtype not in _EDGE_KINDS or images.dim() not in (2, 3):
        raise ValueError("edge_sfr takes a CUDA tensor [H, W] or [B, H, W] of uint8, float32 or float64")
    if side not in ("left", "right"):
        raise ValueError("side must be 'left' or 'right'")
    one = images.dim() == 2
    x = images[None] if one else images
    B, H, W = (int(v) for v in x.shape)
    if min(B, H, W) <= 0:
        raise ValueError("edge_sfr: empty input")
    item_pitch, row_pitch, col = (int(s) for s in x.stride())
    if (W > 1 and col != 1) or (H > 1 and row_pitch < W) or (B > 1 and item_pitch < (H - 1) * max(row_pitch, W) + W):
        raise ValueError("edge_sfr: columns must be adjacent, rows and items must not overlap (take a ROI as frames[:, r0:r1, c0:c1])")
    row_pitch = max(row_pitch, W) if H > 1 else W
    lib = _lib.load()
    block = torch.empty(B * (EDGE_SUMMARY + 3 * EDGE_MAX_BINS) + (B + 1) // 2, dtype=torch.float64, device=x.device)
    out = EdgeSfr(block, B, one, None)
    ws = api._ws(lib.srx_edge_sfr_scratch_bytes(B, H, W))
    out._keep = (x, ws[0])
    _lib.check(getattr(lib, "srx_edge_sfr_" + _EDGE_KINDS[x.dtype])(api._p(x), B, H, W, row_pitch, max(item_pitch, 0), 0 if side == "left" else 1,
                                                                     float(sigma), api._p(out.summary), api._p(out.esf), api._p(out.mtf),
                                                                     api._p(out.status), ws[1], ws[2], api._stream()), "srx_edge_sfr")
    return out


def local_contrast_device(profile, window=16):
    """local_contrast without the copy back: profile [B, n] on the device -> float64 device tensor [B, n]"""
    p, _ = _image(profile, "f64")
    out = torch.empty_like(p)
    _lib.check(_lib.load().srx_local_contrast_f64(api._p(p), p.shape[0], p.shape[1], int(window), api._p(out), api._stream()), "srx_local_contrast")
    return out


def _roi2(img, factor):
    (r0, r1), (c0, c1) = metrics.ROI2_LR
    return img[r0 * factor:r1 * factor, c0 * factor:c1 * factor]


def _profile1(img, factor):
    return img[metrics.ROI1_ROWS_LR[0] * factor:metrics.ROI1_ROWS_LR[1] * factor, metrics.ROI1_COL_LR * factor]


def report_from_sfr(titles, sfr_items, contrast, factor=2):
    """cal_target_report's dict from edge_sfr's items and the local-contrast rows of the profiles (host arrays): frequencies scaled to
    cycles/mm here"""
    hr_pitch = metrics.SENSOR_PITCH_MM / factor
    out = {}
    for title, it, ct in zip(titles, sfr_items, contrast):
        if it["status"] != 0:
            raise RuntimeError(f"{title}: {EDGE_STATUS.get(it['status'], 'edge_sfr status ' + str(it['status']))}")
        out[title] = {"mtf50": it["mtf50"] / hr_pitch, "mtf10": it["mtf10"] / hr_pitch, "edge_angle_deg": it["angle_deg"],
                      "mean_contrast": float(ct[8:-8].mean())}
    return out


def cal_target_report(images, factor=2, side="left", fused=False):
    """metrics.cal_target_report on DEVICE images ({title: CUDA tensor [1536 f, 2048 f] holding the values the PNG gets, i.e. already
    clamped and truncated to 0..255}): MTF50 / MTF10 of the slanted edge in ROI 2, the mean local Michelson contrast of the bar
    cross-section in ROI 1 -- the notebook's summary (analysis.ipynb cells 3-10) -- without reading the PNGs back.
    fused: the ROIs of all images go through ONE edge_sfr call and the profiles through one local-contrast call, with one copy back each
    (the default runs slanted_edge_esf per image, with its four round trips); the same dict within rounding."""
    hr_pitch = metrics.SENSOR_PITCH_MM / factor
    out = {}
    if fused:
        for title, img in images.items():
            if tuple(img.shape) != (1536 * factor, 2048 * factor):
                raise ValueError(f"{title}: the notebook's ROIs are defined on the {1536 * factor} x {2048 * factor} cal-target frame")
        imgs = [img if img.dtype in _EDGE_KINDS else img.to(torch.float64) for img in images.values()]
        if len({i.dtype for i in imgs}) > 1:
            imgs = [i.to(torch.float64) for i in imgs]
        sfr = edge_sfr(torch.stack([_roi2(i.to(api._device()), factor) for i in imgs]), side=side)
        ct = local_contrast_device(torch.stack([_profile1(i.to(api._device()), factor) for i in imgs]), window=16)
        return report_from_sfr(list(images), sfr.result(), ct.cpu().numpy(), factor)
    for title, img in images.items():
        if tuple(img.shape) != (1536 * factor, 2048 * factor):
            raise ValueError(f"{title}: the notebook's ROIs are defined on the {1536 * factor} x {2048 * factor} cal-target frame")
        (r0, r1), (c0, c1) = metrics.ROI2_LR
        roi = img[r0 * factor:r1 * factor, c0 * factor:c1 * factor]
        ex, ey, ang = slanted_edge_esf(roi, side=side)
        fr, mtf, _ = metrics.esf_to_mtf(ex, ey)
        fc = fr / hr_pitch
        v = fc > 0
        prof = img[metrics.ROI1_ROWS_LR[0] * factor:metrics.ROI1_ROWS_LR[1] * factor, metrics.ROI1_COL_LR * factor]
        ct = local_contrast(prof, window=16)
        out[title] = {"mtf50": float(metrics.mtf_at_fraction(fc[v], mtf[v], 0.5)), "mtf10": float(metrics.mtf_at_fraction(fc[v], mtf[v], 0.1)),
                      "edge_angle_deg": float(ang), "mean_contrast": float(ct[8:-8].mean())}
    return out
