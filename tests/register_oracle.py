"""Independent float64 numpy / scipy restatement of srx_register_* (include/srx.h): translation-only sub-pixel registration of
frames against a reference frame.  It is written from the algorithm's statement, not from the kernels:

  crop      the reference crop [m, H - m) x [m, W - m), m = border + search + 2
  coarse    zero-mean NCC of the crop against frame k at every integer offset d = c0 + (oy, ox), |oy|, |ox| <= search, around
            c0 = rint(init_k - init_ref); frame samples outside the frame take the nearest edge value.  A crop with variance
            <= 1e-10 sum t^2 scores 0.  The argmax keeps the first maximum in the order (|dy| + |dx|, dy, dx).
  refine    Gauss-Newton on sum (t(i + d) - r(i))^2, t(i + d) the cubic B-spline interpolant of frame k ('nearest' edges: scipy's
            12-sample edge pad, spline_filter mode 'nearest', tap indices clamped), its analytic gradient from the derivative
            weights; the step -A^-1 g is clamped to +-0.5 px per axis; a frame freezes once max |step| < tol or after n_iter steps.
            det A <= 1e-6 (trace A)^2 or trace A <= 1e-10 sum w^2 -> singular: the frame keeps its coarse shift.
  status    0 ok, 1 singular, 2 coarse argmax on the search boundary, 3 not converged (priority in that order)
  score     zero-mean NCC of t(i + d) against the crop at the returned d (0 when either is constant)

frames[k] ~ ndi.shift(frames[ref], d_k): the sign convention of shifts_yx.
"""
import numpy as np
from scipy import ndimage as ndi

NPAD = 12
VAR_EPS, DET_EPS, GRAD_EPS = 1e-10, 1e-6, 1e-10


def margin(border, search):
    return border + search + 2


def coefficients(frame):
    """cubic B-spline coefficients of the frame with scipy's 'nearest' pre-pad: [H + 24, W + 24]"""
    return ndi.spline_filter(np.pad(np.asarray(frame, np.float64), NPAD, mode="edge"), order=3, mode="nearest")


def _weights(t):
    z = 1.0 - t
    w = np.array([z ** 3 / 6.0, (3 * t ** 3 - 6 * t ** 2 + 4) / 6.0, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6.0, t ** 3 / 6.0])
    dw = np.array([-0.5 * z * z, 1.5 * t * t - 2.0 * t, -1.5 * t * t + t + 0.5, 0.5 * t * t])
    return w, dw


def sample(coef, H, W, m, d):
    """(w, gy, gx) on the crop [m, H - m) x [m, W - m) at positions i + d"""
    idx = []
    for ax, n in ((0, H), (1, W)):
        fl = np.floor(d[ax])
        w, dw = _weights(d[ax] - fl)
        base = np.arange(m, n - m) + int(fl) + NPAD - 1
        taps = [np.clip(base + a, 0, n + 2 * NPAD - 1) for a in range(4)]
        idx.append((w, dw, taps))
    (wy, dwy, ty), (wx, dwx, tx) = idx
    hx = [sum(wx[b] * coef[np.ix_(ty[a], tx[b])] for b in range(4)) for a in range(4)]
    dhx = [sum(dwx[b] * coef[np.ix_(ty[a], tx[b])] for b in range(4)) for a in range(4)]
    return (sum(wy[a] * hx[a] for a in range(4)), sum(dwy[a] * hx[a] for a in range(4)), sum(wy[a] * dhx[a] for a in range(4)))


def ncc(t, r):
    n = t.size
    st, sr = t.sum(), r.sum()
    vt, vr = (t * t).sum() - st * st / n, (r * r).sum() - sr * sr / n
    if not (vt > VAR_EPS * (t * t).sum()) or not (vr > VAR_EPS * (r * r).sum()):
        return 0.0
    return float(((t * r).sum() - st * sr / n) / np.sqrt(vt * vr))


def coarse(t, r_crop, m, c0, search):
    """-> (dy, dx) integer, on_boundary"""
    H, W = t.shape
    ys, xs = np.arange(m, H - m), np.arange(m, W - m)
    best = None
    for oy in range(-search, search + 1):
        for ox in range(-search, search + 1):
            dy, dx = c0[0] + oy, c0[1] + ox
            tc = t[np.ix_(np.clip(ys + dy, 0, H - 1), np.clip(xs + dx, 0, W - 1))]
            key = (-ncc(tc, r_crop), abs(dy) + abs(dx), dy, dx)
            if best is None or key < best[0]:
                best = (key, oy, ox)
    _, oy, ox = best
    return (c0[0] + oy, c0[1] + ox), search > 0 and (abs(oy) == search or abs(ox) == search)


def register_item(frames, ref=0, init=None, search=2, border=8, n_iter=10, tol=1e-4):
    """frames [N, H, W] -> (d [N, 2], score [N], status [N], d_coarse [N, 2])"""
    frames = np.asarray(frames, np.float64)
    N, H, W = frames.shape
    m = margin(border, search)
    assert H - 2 * m >= 16 and W - 2 * m >= 16
    init = np.zeros((N, 2)) if init is None else np.asarray(init, np.float64).reshape(N, 2)
    r = frames[ref][m:H - m, m:W - m]
    d_out, score, status, d_co = np.zeros((N, 2)), np.ones(N), np.zeros(N, np.int32), np.zeros((N, 2))
    for k in range(N):
        if k == ref:
            continue
        c0 = tuple(int(v) for v in np.rint(init[k] - init[ref]))
        dc, edge = coarse(frames[k], r, m, c0, search)
        d = np.array(dc, np.float64)
        d_co[k] = d
        coef = coefficients(frames[k])
        st, steps, last = 0, 0, 0.0
        while steps < n_iter:
            w, gy, gx = sample(coef, H, W, m, d)
            e = w - r
            a, b, c = (gy * gy).sum(), (gy * gx).sum(), (gx * gx).sum()
            g0, g1 = (gy * e).sum(), (gx * e).sum()
            det = a * c - b * b
            if not (det > DET_EPS * (a + c) * (a + c)) or not (a + c > GRAD_EPS * (w * w).sum()):
                d, st = np.array(dc, np.float64), 1
                break
            sy = np.clip(-(c * g0 - b * g1) / det, -0.5, 0.5)
            sx = np.clip(-(a * g1 - b * g0) / det, -0.5, 0.5)
            d = d + np.array([sy, sx])
            steps += 1
            last = max(abs(sy), abs(sx))
            if last < tol:
                break
        if st == 0:
            st = 2 if edge else (3 if n_iter > 0 and last >= tol else 0)
        w = sample(coef, H, W, m, d)[0]
        d_out[k], score[k], status[k] = d, ncc(w, r), st
    return d_out, score, status, d_co
