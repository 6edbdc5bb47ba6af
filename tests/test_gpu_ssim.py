"""Device SSIM (srx_ssim_*: one pass over the pair, sr_mi355x.metrics_device.ssim / ssim_affine / ecc) against the independent oracle of
tests/ssim_oracle.py and against the host forms: windows, radii, constants, crops, odd shapes, batches, maps with their reflect-influenced
rim, closed forms, symmetry, determinism and the workspace bound."""
import ctypes

import numpy as np
import pytest
import torch

import ssim_oracle as O
from sr_mi355x import _lib, api
from sr_mi355x import metrics as M
from sr_mi355x import metrics_device as D

pytestmark = pytest.mark.gpu

# float64: the oracle's own precision (differences are summation order).  float32: a window sum of squares of 8-bit values (up to
# 255^2 = 65025, eps 6e-8) carries ~4e-3 of rounding into a variance, and S divides it by vx + vy + C2 >= C2 = 58.5: up to ~1e-4 per
# pixel.  Observed on these pairs: 1.1e-4 at worst (a 3 x 3 window, where the variances are smallest), so the map is held to 2e-4;
# the mean averages those errors out and keeps 1e-5.
TOL = {torch.float64: (1e-12, 1e-10), torch.float32: (1e-5, 2e-4)}


def pair(h, w, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w)).astype(np.float64)
    # smooth structure plus noise: local variances from ~0 to large, SSIM well inside (0, 1)
    yy, xx = np.mgrid[:h, :w]
    a = np.clip(0.5 * a + 100 * np.sin(xx / 7.0) * np.cos(yy / 11.0) + 100, 0, 255).round()
    b = np.clip(0.7 * a + 0.3 * np.roll(a, 2, axis=0) + rng.normal(0, 10, (h, w)) + 5, 0, 255).round()
    return a, b


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dt)


def oracle_kw(kw):
    return dict(win_size=kw.get("win_size"), gaussian=kw.get("gaussian_weights", False), sigma=kw.get("sigma", 1.5),
                sample_cov=kw.get("use_sample_covariance", True), K1=kw.get("K1", 0.01), K2=kw.get("K2", 0.03),
                border=kw.get("border", 0), data_range=kw.get("data_range", 255.0))


CASES = [dict(), dict(gaussian_weights=True), dict(win_size=3), dict(win_size=15), dict(use_sample_covariance=False),
         dict(K1=0.02, K2=0.05), dict(border=10), dict(gaussian_weights=True, sigma=0.9, border=3), dict(win_size=5, data_range=300.0)]
SHAPES = [(61, 97), (300, 517), (15, 300)]


def _fits(kw, shape):
    win = kw.get("win_size", 11 if kw.get("gaussian_weights") and kw.get("sigma", 1.5) == 1.5 else 7)
    return min(shape) - 2 * kw.get("border", 0) >= win


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
@pytest.mark.parametrize("kw,shape", [(kw, s) for kw in CASES for s in SHAPES if _fits(kw, s)])
def test_mean_and_map_match_the_oracle(dt, kw, shape):
    h, w = shape
    kw = dict(kw)
    a, b = pair(h, w, seed=h + w)
    om, omap = O.ssim(a, b, **oracle_kw(kw))
    dr = kw.pop("data_range", 255.0)
    m, smap = D.ssim(dev(a, dt), dev(b, dt), data_range=dr, full=True, **kw)
    tm, tmap = TOL[dt]
    assert smap.dtype == dt and tuple(smap.shape) == omap.shape
    assert abs(m - om) <= tm, (m, om)
    assert np.abs(smap.double().cpu().numpy() - omap).max() <= tmap
    assert D.ssim(dev(a, dt), dev(b, dt), data_range=dr, **kw) == m  # without the map: same partial sums


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_data_range_one_and_uint8_default(dt):
    a, b = pair(80, 90, seed=2)
    om = O.ssim(a, b)[0]
    assert abs(D.ssim(dev(a / 255.0, dt), dev(b / 255.0, dt), data_range=1.0) - om) <= TOL[dt][0]
    u8 = D.ssim(torch.from_numpy(a.astype(np.uint8)).cuda(), torch.from_numpy(b.astype(np.uint8)).cuda())  # data_range 255, float64
    assert abs(u8 - om) <= 1e-12
    with pytest.raises(ValueError):
        D.ssim(dev(a, dt), dev(b, dt))


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_window_sized_images(dt):
    for (h, w), kw in (((7, 7), {}), ((3, 3), dict(win_size=3)), ((15, 40), dict(win_size=15)), ((11, 11), dict(gaussian_weights=True))):
        a, b = pair(h, w, seed=h * w)
        om, omap = O.ssim(a, b, **oracle_kw(kw))
        m, smap = D.ssim(dev(a, dt), dev(b, dt), data_range=255.0, full=True, **kw)
        assert abs(m - om) <= TOL[dt][0] and np.abs(smap.double().cpu().numpy() - omap).max() <= TOL[dt][1], (h, w, kw)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_batch_of_three_different_pairs(dt):
    ps = [pair(131, 277, seed=s) for s in (10, 11, 12)]
    ps[2] = (ps[2][0], ps[2][0][::-1].copy())  # a poor match as well
    A = dev(np.stack([p[0] for p in ps]), dt)
    Bt = dev(np.stack([p[1] for p in ps]), dt)
    for kw in (dict(), dict(gaussian_weights=True, border=10)):
        ms, maps = D.ssim(A, Bt, data_range=255.0, full=True, **kw)
        assert isinstance(ms, list) and len(ms) == 3 and tuple(maps.shape)[0] == 3
        for i, (a, b) in enumerate(ps):
            om, omap = O.ssim(a, b, **oracle_kw(kw))
            assert abs(ms[i] - om) <= TOL[dt][0]
            assert np.abs(maps[i].double().cpu().numpy() - omap).max() <= TOL[dt][1]
            assert abs(D.ssim(A[i], Bt[i], data_range=255.0, **kw) - ms[i]) <= TOL[dt][0]  # an item alone (its own block grid)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_closed_forms_symmetry_and_determinism(dt):
    a, b = pair(200, 333, seed=4)
    A, Bt = dev(a, dt), dev(b, dt)
    assert D.ssim(A, A, data_range=255.0) >= 1 - (1e-12 if dt == torch.float64 else 1e-6)
    c1, c2 = 40.0, 170.0
    C1 = (0.01 * 255) ** 2
    want = (2 * c1 * c2 + C1) / (c1 * c1 + c2 * c2 + C1)
    got = D.ssim(torch.full((50, 60), c1, dtype=dt, device="cuda"), torch.full((50, 60), c2, dtype=dt, device="cuda"), data_range=255.0)
    assert abs(got - want) <= (1e-14 if dt == torch.float64 else 1e-6)
    for kw in (dict(), dict(gaussian_weights=True), dict(win_size=15, border=7)):
        ab, maba = D.ssim(A, Bt, data_range=255.0, full=True, **kw)
        ba, mbab = D.ssim(Bt, A, data_range=255.0, full=True, **kw)
        assert ab == ba and torch.equal(maba, mbab)  # bit-identical
        assert D.ssim(A, Bt, data_range=255.0, **kw) == ab  # run to run


@pytest.mark.parametrize("prec,dt", [("f64", torch.float64), ("f32", torch.float32)])
def test_exact_metrics_workspace_suffices(prec, dt):
    B, H, W = 2, 96, 1000
    ps = [pair(H, W, seed=s) for s in (20, 21)]
    A, Bt = dev(np.stack([p[0] for p in ps]), dt), dev(np.stack([p[1] for p in ps]), dt)
    lib = _lib.load()
    n = lib.srx_metrics_workspace_bytes(B, H, W, 1)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(B, dtype=torch.float64, device="cuda")
    k = np.full(7, 1.0 / 7)
    fn = getattr(lib, f"srx_ssim_{prec}")
    st = fn(api._p(A), api._p(Bt), B, H, W, 0, 3, k.ctypes.data_as(_lib._HD), 1, 255.0, 0.01, 0.03, None, api._p(out), None,
            api._p(ws), ctypes.c_size_t(n), api._stream())
    assert st == _lib.OK
    got = out.cpu().numpy()
    for i, (a, b) in enumerate(ps):
        assert abs(got[i] - O.ssim(a, b)[0]) <= TOL[dt][0]


@pytest.mark.parametrize("dt", [torch.float64, torch.float32])
def test_ssim_affine_and_ecc_match_the_host_forms(dt):
    a, b = pair(150, 210, seed=8)
    b = np.clip(0.5 * b + 60, 0, 255).round()  # a contrast / brightness change for the fit to undo
    A, Bt = dev(a, dt), dev(b, dt)
    tm = 1e-10 if dt == torch.float64 else TOL[dt][0]
    assert abs(D.ssim_affine(A, Bt) - M.ssim_affine(a, b)) <= tm
    assert abs(D.ssim_affine(A, Bt, border=0, gaussian_weights=True) - M.ssim_affine(a, b, border=0, gaussian_weights=True)) <= tm
    assert abs(M.ssim_affine(a, b) - O.ssim_affine(a, b)) <= 1e-10
    for border in (0, 10):
        assert abs(D.ecc(A, Bt, border=border) - M.ecc(a, b, border=border)) <= 1e-12
    both = D.ecc(torch.stack([A, A]), torch.stack([Bt, A]))
    assert isinstance(both, list) and abs(both[0] - M.ecc(a, b)) <= 1e-12 and abs(both[1] - 1.0) <= 1e-12
    aff = D.ssim_affine(torch.stack([A, A]), torch.stack([Bt, A]))
    assert abs(aff[0] - M.ssim_affine(a, b)) <= tm and aff[1] >= 1 - 1e-6


def test_full_frame_float32_against_the_float64_oracle():
    """A 3072 x 4096 pair of 8-bit values (the cal-target HR frame) in float32 against the float64 oracle."""
    rng = np.random.default_rng(99)
    h, w = 3072, 4096
    yy, xx = np.mgrid[:h, :w]
    a = np.clip(128 + 100 * np.sin(xx / 23.0) * np.sign(np.cos(yy / 37.0)) + rng.normal(0, 6, (h, w)), 0, 255).round()
    b = np.clip(0.8 * a + 20 + rng.normal(0, 8, (h, w)), 0, 255).round()
    om, _ = O.ssim(a, b)
    m = D.ssim(dev(a, torch.float32), dev(b, torch.float32), data_range=255.0)
    assert abs(m - om) <= 1e-5, (m, om)
    m64 = D.ssim(dev(a, torch.float64), dev(b, torch.float64), data_range=255.0)
    assert abs(m64 - om) <= 1e-12, (m64, om)
