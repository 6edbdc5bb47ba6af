"""The numpy reference of the patch grid, the gather and the blend (srx_patches_*, include/srx.h), shared by tests/test_patchwise_host.py
and tests/test_gpu_patchwise.py, and the analytic field-test input (a truth image of cosines seen through a shift that varies over the
field).  A plain helper module: no fixtures, nothing registered.

The blend is computed in the dtype of the patches with the operation order the header fixes: the integer weight product converted once,
each term rounded once, the terms added in ascending (i, j) with plain additions, one division.  (Terms of weight 0 are added here and
skipped on the device: x + (+-0) is x for every partial sum, which starts at +0 and therefore is never -0.)"""
import numpy as np


def count(n, L, s):
    return -(-(n - L) // s) + 1


def origins(n, L, s):
    return [min(i * s, n - L) for i in range(count(n, L, s))]


def accepted(n, L, s):
    """the axis arguments the entry points accept (srx_patches_count is 0 for the others)"""
    return n > 0 and 0 < L <= n and 0 < s <= L and 2 * s >= L


def weights(n, L, s, margin):
    """int64 [count, L]: the weight of patch i at the coordinate o_i + t"""
    R = L - s - 2 * margin
    out = np.zeros((count(n, L, s), L), np.int64)
    for i, o in enumerate(origins(n, L, s)):
        x = o + np.arange(L)
        dl = x - o + 1 - margin if o > 0 else np.full(L, R)
        dr = o + L - x - margin if o + L < n else np.full(L, R)
        out[i] = np.clip(np.minimum(dl, dr), 0, R)
    return out


def weight_sums(n, L, s, margin):
    """(S int64 [n]: the sum of the weights over x; cover int64 [n]: the patches that contain x)"""
    S, cover = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for o, wi in zip(origins(n, L, s), weights(n, L, s, margin)):
        S[o:o + L] += wi
        cover[o:o + L] += 1
    return S, cover


def gather(frames, ph, pw, sy, sx):
    """[B, N, h, w] -> [B P, N, ph, pw], plain slicing"""
    B, N, h, w = frames.shape
    oy, ox = origins(h, ph, sy), origins(w, pw, sx)
    out = np.empty((B * len(oy) * len(ox), N, ph, pw), frames.dtype)
    k = 0
    for b in range(B):
        for y in oy:
            for x in ox:
                out[k] = frames[b, :, y:y + ph, x:x + pw]
                k += 1
    return out


def blend(patches, H, W, SY, SX, margin):
    """[B P, PH, PW] -> [B, H, W] in the dtype of `patches`"""
    T = patches.dtype.type
    BP, PH, PW = patches.shape
    oy, ox = origins(H, PH, SY), origins(W, PW, SX)
    P = len(oy) * len(ox)
    assert BP % P == 0
    wy, wx = weights(H, PH, SY, margin), weights(W, PW, SX, margin)
    Sy, _ = weight_sums(H, PH, SY, margin)
    Sx, _ = weight_sums(W, PW, SX, margin)
    den = (Sy[:, None] * Sx[None, :]).astype(T)
    out = np.empty((BP // P, H, W), T)
    for b in range(BP // P):
        acc = np.zeros((H, W), T)
        for i, y in enumerate(oy):
            for j, x in enumerate(ox):
                wgt = (wy[i][:, None] * wx[j][None, :]).astype(T)
                term = wgt * patches[b * P + i * len(ox) + j]
                acc[y:y + PH, x:x + PW] = acc[y:y + PH, x:x + PW] + term
        out[b] = acc / den
    return out


def random_patches(B, H, W, PH, PW, SY, SX, dtype, seed):
    """patches with fractions (every product and sum rounds) and both signs"""
    rng = np.random.default_rng(seed)
    P = count(H, PH, SY) * count(W, PW, SX)
    return (rng.uniform(-40.0, 300.0, (B * P, PH, PW)) / 3.0).astype(dtype)


# name: (B, H, W, PH, PW, SY, SX, margin) -- the blend cases of the host model and of the GPU test
BLEND_CASES = {
    "300x342_L128_s96_m0": (1, 300, 342, 128, 128, 96, 96, 0),     # odd width, clamped last origin on both axes
    "300x342_L128_s96_m8": (1, 300, 342, 128, 128, 96, 96, 8),
    "s_half_L_three_cover": (1, 65, 97, 32, 32, 16, 16, 0),        # n = 2 L + 1 rows: three patches over the samples 32 .. 47
    "s_half_L_three_cover_m3": (1, 65, 97, 32, 32, 16, 16, 3),
    "single_patch_rows": (1, 48, 101, 48, 64, 32, 40, 2),          # H = PH: one patch on the row axis; patches are not square
    "single_patch_both": (1, 40, 40, 40, 40, 24, 24, 1),
    "B2_70x83": (2, 70, 83, 32, 32, 24, 20, 2),                    # two images; strides differ between the axes
}


def blend_case(name, dtype):
    B, H, W, PH, PW, SY, SX, margin = BLEND_CASES[name]
    return random_patches(B, H, W, PH, PW, SY, SX, dtype, seed=sorted(BLEND_CASES).index(name) + 5)


# ---------------------------------------------------------------------------------------------------------------------------------
# field test: analytic frames under a shift that varies over the field
# ---------------------------------------------------------------------------------------------------------------------------------
FIELD_H, FIELD_W, FIELD_F = 160, 192, 2
FIELD_SLOPE = 0.4


def field_terms():
    rng = np.random.default_rng(459)
    n = 60
    u, v = rng.uniform(-0.15, 0.15, n), rng.uniform(-0.15, 0.15, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    A = rng.uniform(2.0, 10.0, n)
    return u, v, phi, A * (220.0 / A.sum())


def field_truth():
    """[2 h, 2 w] float64"""
    u, v, phi, A = field_terms()
    y, x = np.mgrid[0:FIELD_F * FIELD_H, 0:FIELD_F * FIELD_W].astype(np.float64)
    img = np.full(y.shape, 127.5)
    for m in range(len(A)):
        img += A[m] * np.cos(2.0 * np.pi * (u[m] * y + v[m] * x) + phi[m])
    return img


def psf_gain(psf, u, v):
    """G_m = sum k[i, j] cos(2 pi (u_m i + v_m j)), i, j counted from the kernel's centre"""
    k = np.asarray(psf, dtype=np.float64)
    i, j = np.mgrid[0:k.shape[0], 0:k.shape[1]].astype(np.float64)
    i, j = i - (k.shape[0] - 1) // 2, j - (k.shape[1] - 1) // 2
    return np.array([(k * np.cos(2.0 * np.pi * (um * i + vm * j))).sum() for um, vm in zip(u, v)])


def field_true_shift(nominal, X):
    """s_k at the LR column X (float, may be an array): nominal_k (1 + 0.4 (2 X / (w - 1) - 1)) -> [..., N, 2]"""
    scale = 1.0 + FIELD_SLOPE * (2.0 * np.asarray(X, dtype=np.float64) / (FIELD_W - 1) - 1.0)
    return np.asarray(nominal, dtype=np.float64) * scale[..., None, None]


def field_frames(nominal, psf, noise=True):
    """uint8 [N, h, w] (noise=False: the float64 frames before noise and rounding)"""
    u, v, phi, A = field_terms()
    G = psf_gain(psf, u, v)
    Y, X = np.mgrid[0:FIELD_H, 0:FIELD_W].astype(np.float64)
    scale = 1.0 + FIELD_SLOPE * (2.0 * X / (FIELD_W - 1) - 1.0)
    frames = []
    for sy0, sx0 in np.asarray(nominal, dtype=np.float64):
        sy, sx = sy0 * scale, sx0 * scale
        fr = np.full(Y.shape, 127.5)
        for m in range(len(A)):
            fr += A[m] * G[m] * np.cos(2.0 * np.pi * (u[m] * (FIELD_F * Y - FIELD_F * sy) + v[m] * (FIELD_F * X - FIELD_F * sx)) + phi[m])
        frames.append(fr)
    frames = np.stack(frames)
    if not noise:
        return frames
    rng = np.random.default_rng(460)
    return np.clip(np.rint(frames + rng.normal(0.0, 1.0, frames.shape)), 0, 255).astype(np.uint8)


def psnr(a, b, border=16, peak=255.0):
    d = (np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))[border:-border, border:-border]
    return 10.0 * np.log10(peak * peak / np.mean(d * d))
