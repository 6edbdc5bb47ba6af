"""Independent numpy oracle of SSIM (skimage.metrics.structural_similarity, 2-D grayscale), of the vendor view's affine-fit SSIM and of
its ECC score, written from the definition and shared by tests/test_ssim_host.py and tests/test_gpu_ssim.py.  It does not use
sr_mi355x: the window sums are one 2-D weighted sum per pixel over a 'symmetric'-padded image (scipy.ndimage's 'reflect'), the window
the outer product of the 1-D taps; test_ssim_host.py checks those sums against scipy.ndimage.uniform_filter / gaussian_filter."""
import numpy as np


def crop(a, border):
    a = np.asarray(a, dtype=np.float64)
    return a[border:a.shape[0] - border, border:a.shape[1] - border]


def taps(win_size=7, gaussian=False, sigma=1.5):
    if gaussian:
        r = int(3.5 * sigma + 0.5)
        x = np.arange(-r, r + 1, dtype=np.float64)
        k = np.exp(-(x * x) / (2.0 * sigma * sigma))
        return k / k.sum()
    return np.full(win_size, 1.0 / win_size)


def window_mean(a, k):
    """sum over the (2r + 1)^2 window of outer(k, k) * a, 'reflect' boundary (d c b a | a b c d)"""
    r = len(k) // 2
    a = np.asarray(a, dtype=np.float64)
    ap = np.pad(a, r, mode="symmetric")
    h, w = a.shape
    out = np.zeros_like(a)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            out += (k[i] * k[j]) * ap[i:i + h, j:j + w]
    return out


def ssim(x, y, win_size=None, data_range=255.0, gaussian=False, sigma=1.5, sample_cov=True, K1=0.01, K2=0.03, border=0):
    """(mean SSIM, S map over the crop)"""
    x, y = crop(x, border), crop(y, border)
    if win_size is None:
        win_size = 2 * int(3.5 * sigma + 0.5) + 1 if gaussian else 7
    k = taps(win_size, gaussian, sigma)
    n = win_size * win_size
    cov = n / (n - 1.0) if sample_cov else 1.0
    ux, uy = window_mean(x, k), window_mean(y, k)
    uxx, uyy, uxy = window_mean(x * x, k), window_mean(y * y, k), window_mean(x * y, k)
    vx, vy, vxy = cov * (uxx - ux * ux), cov * (uyy - uy * uy), cov * (uxy - ux * uy)
    c1, c2 = (K1 * data_range) ** 2, (K2 * data_range) ** 2
    s = (2.0 * ux * uy + c1) * (2.0 * vxy + c2) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    p = (win_size - 1) // 2
    return float(s[p:s.shape[0] - p, p:s.shape[1] - p].mean(dtype=np.float64)), s


def ssim_affine(ref, test, border=10, data_range=1.0, **kw):
    """crop, scale by 1/255, least-squares test -> a test + b (normal equations), SSIM of ref against the fitted test"""
    r, t = crop(ref, border) / 255.0, crop(test, border) / 255.0
    A = np.stack([t.ravel(), np.ones(t.size)], axis=1)
    (a, b), *_ = np.linalg.lstsq(A, r.ravel(), rcond=None)
    return ssim(r, a * t + b, data_range=data_range, **kw)[0]


def ecc(ref, test, border=0):
    r, t = crop(ref, border), crop(test, border)
    r, t = r - r.mean(), t - t.mean()
    return float((r * t).sum() / np.sqrt((r * r).sum() * (t * t).sum()))
