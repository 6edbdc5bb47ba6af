"""SSIM / ECC host forms (sr_mi355x.metrics.ssim, ssim_affine, ecc) against an independent oracle (tests/ssim_oracle.py), the oracle
against the scipy.ndimage filters skimage's structural_similarity calls, the window / data_range checks, and the argument checks of
srx_ssim_* that need no GPU."""
import ctypes

import numpy as np
import pytest

import ssim_oracle as O
from sr_mi355x import _lib
from sr_mi355x import metrics as M


def pair(h, w, seed=0, dtype=np.uint8):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w))
    # a smoothed, noisy, brightness-shifted copy: a realistic reconstruction-vs-reference pair, SSIM well inside (0, 1)
    b = np.clip(0.6 * a + 0.4 * np.roll(a, 1, axis=1) + rng.normal(0, 12, (h, w)) + 9, 0, 255)
    return a.astype(dtype), np.round(b).astype(dtype)


@pytest.mark.parametrize("shape", [(7, 9), (23, 31), (64, 50)])
def test_oracle_window_sums_match_scipy(shape):
    nd = pytest.importorskip("scipy.ndimage")
    a = np.random.default_rng(1).random(shape) * 255
    assert np.abs(O.window_mean(a, O.taps(7)) - nd.uniform_filter(a, size=7, mode="reflect")).max() < 1e-11
    assert np.abs(O.window_mean(a, O.taps(3)) - nd.uniform_filter(a, size=3, mode="reflect")).max() < 1e-11
    for sigma in (1.5, 0.8):
        want = nd.gaussian_filter(a, sigma=sigma, truncate=3.5, mode="reflect")
        assert np.abs(O.window_mean(a, O.taps(gaussian=True, sigma=sigma)) - want).max() < 1e-11


def test_oracle_ssim_matches_the_scipy_recipe():
    """skimage's structural_similarity restated on scipy.ndimage filters (filter of x, y, x^2, y^2, x y, then the formula)."""
    nd = pytest.importorskip("scipy.ndimage")
    a, b = pair(40, 57)
    x, y = a.astype(np.float64), b.astype(np.float64)
    for filt, win in ((lambda z: nd.uniform_filter(z, size=7), 7), (lambda z: nd.gaussian_filter(z, sigma=1.5, truncate=3.5), 11)):
        ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
        cn = win * win / (win * win - 1.0)
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        s = (2 * ux * uy + c1) * (2 * vxy + c2) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        p = (win - 1) // 2
        m, smap = O.ssim(a, b, gaussian=win == 11)
        assert abs(m - s[p:-p, p:-p].mean()) < 1e-12
        assert np.abs(smap - s).max() < 1e-10


CASES = [dict(), dict(gaussian_weights=True), dict(win_size=3), dict(win_size=15), dict(use_sample_covariance=False),
         dict(K1=0.02, K2=0.05), dict(border=10), dict(gaussian_weights=True, sigma=0.9, border=3)]


@pytest.mark.parametrize("kw", CASES)
def test_host_ssim_matches_the_oracle(kw):
    a, b = pair(45, 61, seed=3)
    m, smap = M.ssim(a, b, full=True, **kw)
    o = dict(win_size=kw.get("win_size"), gaussian=kw.get("gaussian_weights", False), sigma=kw.get("sigma", 1.5),
             sample_cov=kw.get("use_sample_covariance", True), K1=kw.get("K1", 0.01), K2=kw.get("K2", 0.03), border=kw.get("border", 0))
    om, omap = O.ssim(a, b, **o)
    assert abs(m - om) < 1e-12 and np.abs(smap - omap).max() < 1e-10
    assert M.ssim(a, b, **kw) == m
    # float input with data_range: the same number on the 0..1 scale
    fm = M.ssim(a / 255.0, b / 255.0, data_range=1.0, **kw)
    assert abs(fm - om) < 1e-12


def test_host_ssim_identity_and_symmetry():
    a, b = pair(30, 30, seed=5)
    assert M.ssim(a, a) >= 1 - 1e-12
    assert M.ssim(a, b) == pytest.approx(M.ssim(b, a), abs=1e-15)


def test_host_ssim_affine_and_ecc():
    a, b = pair(60, 70, seed=7)
    assert abs(M.ssim_affine(a, b) - O.ssim_affine(a, b)) < 1e-10
    assert abs(M.ssim_affine(a, b, border=0, gaussian_weights=True) - O.ssim_affine(a, b, border=0, gaussian=True)) < 1e-10
    for border in (0, 10):
        e = M.ecc(a, b, border=border)
        assert abs(e - O.ecc(a, b, border)) < 1e-12
        assert abs(e - np.corrcoef(O.crop(a, border).ravel(), O.crop(b, border).ravel())[0, 1]) < 1e-12
    assert M.ecc(a, a) == pytest.approx(1.0, abs=1e-14)
    assert np.isnan(M.ecc(a, np.full_like(a, 7)))


def test_window_and_range_are_checked():
    a, b = pair(20, 25)
    for bad in (4, 1, 2, 21, 27):
        with pytest.raises(ValueError):
            M.ssim(a, b, win_size=bad)
    with pytest.raises(ValueError):
        M.ssim(a, b, win_size=11, border=5)  # 10 x 15 crop
    with pytest.raises(ValueError):
        M.ssim(a.astype(np.float64), b.astype(np.float64))  # float without data_range
    with pytest.raises(ValueError):
        M.ssim(a, b, gaussian_weights=True, win_size=7)  # sigma 1.5 fixes the Gaussian window at 11
    with pytest.raises(ValueError):
        M.ssim(a, b[:, :-1])
    assert M.ssim(a, b, win_size=19) == pytest.approx(O.ssim(a, b, win_size=19)[0], abs=1e-12)  # the largest window that fits


def test_ssim_argument_checks_without_gpu():
    """Invalid arguments are SRX_E_INVALID, a radius past 7 SRX_E_UNSUPPORTED, before any HIP call (the pointers are never used)."""
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    k7 = np.full(7, 1.0 / 7)
    k17 = np.full(17, 1.0 / 17)
    kp, k17p = k7.ctypes.data_as(_lib._HD), k17.ctypes.data_as(_lib._HD)
    ws = 1 << 20
    for fn in (lib.srx_ssim_f32, lib.srx_ssim_f64):
        ok = dict(ref=fake, test=fake, B=1, H=32, W=32, border=0, radius=3, taps=kp, cov=1, dr=255.0, k1=0.01, k2=0.03, aff=None, out=fake,
                  map=None, ws=fake, wsb=ws, st=None)

        def call(**kw):
            a = dict(ok, **kw)
            return fn(*a.values())
        assert call(ref=None) == _lib.E_INVALID
        assert call(test=None) == _lib.E_INVALID
        assert call(taps=None) == _lib.E_INVALID
        assert call(out=None) == _lib.E_INVALID
        assert call(B=0) == _lib.E_INVALID
        assert call(H=0) == _lib.E_INVALID
        assert call(border=-1) == _lib.E_INVALID
        assert call(border=16) == _lib.E_INVALID
        assert call(radius=0) == _lib.E_INVALID
        assert call(dr=0.0) == _lib.E_INVALID
        assert call(dr=float("nan")) == _lib.E_INVALID
        assert call(k1=float("inf")) == _lib.E_INVALID
        assert call(H=6, W=40) == _lib.E_INVALID           # window 7 taller than the image
        assert call(border=13) == _lib.E_INVALID           # 6 x 6 crop
        assert call(radius=8, taps=k17p) == _lib.E_UNSUPPORTED
        assert call(radius=8, taps=k17p, H=100, W=100, ws=None, wsb=0) == _lib.E_UNSUPPORTED
        assert call(ws=None, wsb=0) == _lib.E_WORKSPACE
