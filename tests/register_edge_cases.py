"""Cases, seeded generators and expected values of the registration edge tests: tests/test_register_edges_host.py checks every
precondition on the oracle of tests/register_oracle.py alone (no GPU), tests/test_gpu_register_edges.py holds srx_register_* and
srx_register_u8_* (include/srx.h) to the same cases.  Host only: numpy, scipy and the oracle.

Every frame is integer-valued in 0..255 and kept as uint8, so a case runs through the float and the byte entry points alike.  Frames come
from a scipy-only recipe -- a Gaussian-filtered uniform field, ndi.shift, sigma-1 noise, rint, clip -- and the exact expectations (ties,
rounding, clamped steps, constant content) do not depend on it; what does is stated as a precondition and asserted by the host test.

case(name) is (frames uint8 [N, H, W], keyword arguments of the call) and oracle(name) the oracle's result on it, each computed once per
process and read-only."""
import functools

import numpy as np
from scipy import ndimage as ndi

import register_oracle as R

SEED = 20251
FORMS = (("float", "f32"), ("float", "f64"), ("u8", "f32"), ("u8", "f64"))
# tests/test_gpu_register.py's: float64 is the oracle's own precision, float32 keeps the frames' coefficients in float32
TOL_SHIFT = {"f64": 1e-8, "f32": 1e-3}
TOL_SCORE = {"f64": 1e-10, "f32": 1e-4}

# csrc/srx_register.hpp
CW, CH, CBLK, GW, GBLK = 64, 16, 256, 256, 256


def cdiv(a, b):
    return -(-a // b)


def make_plan(h, w, search):
    """make_plan of csrc/srx_register.hpp restated for a crop h x w: the coarse grid (cgx, cgy), its rows per block, the refinement grid"""
    cgx = cdiv(w, CW)
    gy = max(1, min(cdiv(CBLK, cgx), cdiv(h, CH)))
    crow = cdiv(cdiv(h, gy), CH) * CH
    ggx = cdiv(w, GW)
    gy = max(1, min(cdiv(GBLK, ggx), cdiv(h, 16)))
    grow = cdiv(h, gy)
    return dict(noff=(2 * search + 1) ** 2, groups=256 // (2 * search + 1) ** 2, cgx=cgx, cgy=cdiv(h, crow), crow=crow, ggx=ggx,
                ggy=cdiv(h, grow), grow=grow)


def crop_of(shape, search, border):
    m = R.margin(border, search)
    return shape[-2] - 2 * m, shape[-1] - 2 * m


# ---- generators -------------------------------------------------------------------------------------------------------------------------
PAD = 16  # the scene is larger than the frame by this much on every side, so a shifted frame has real content at its edges


def scene(h, w, seed, sigma=2.0):
    """float64 [h + 2 PAD, w + 2 PAD] in 20..235: a Gaussian-filtered uniform field"""
    u = ndi.gaussian_filter(np.random.default_rng([SEED, seed]).uniform(0.0, 1.0, (h + 2 * PAD, w + 2 * PAD)), sigma)
    return 20.0 + 215.0 * (u - u.min()) / (u.max() - u.min())


def frames_of(h, w, shifts, seed, sigma=2.0):
    """uint8 [N, h, w]: frame k ~ ndi.shift(frame 0's scene, shifts[k]), noise sigma 1, rint, clip"""
    base = scene(h, w, seed, sigma)
    fr = np.stack([ndi.shift(base, s, order=3, mode="nearest")[PAD:-PAD, PAD:-PAD] for s in shifts])
    fr = fr + np.random.default_rng([SEED, seed, 1]).normal(0.0, 1.0, fr.shape)
    return np.clip(np.rint(fr), 0, 255).astype(np.uint8)


def u8(a):
    a = np.ascontiguousarray(a)
    assert np.array_equal(a, np.clip(np.rint(a), 0, 255))
    return a.astype(np.uint8)


# ---- 1a. ties of the coarse argmax ------------------------------------------------------------------------------------------------------
TIE_KW = dict(search=4, border=8)
TIE_ROLLS = [(0, 0), (2, 2), (1, 0), (2, 0), (0, 2), (2, 1), (3, 2)]
TIE_EXPECT = [(0, 0), (-2, -2), (1, 0), (-2, 0), (0, -2), (-2, 1), (-1, -2)]
TIE_MAXIMA = {(0, 0): 9, (3, 2): 4}  # the number of tied maxima the issue names
TIE2_KW = dict(search=2, border=8, init=[[0.0, 0.0], [-3.0, 0.0], [0.0, 3.0]])
TIE2_ROLLS = [(-1, 0), (0, 1)]
TIE2_EXPECT = [(-1, 0), (0, 1)]
TIE_GAP = 0.05


def tie_base():
    return np.tile(np.random.default_rng(11).integers(0, 256, (4, 4)), (16, 16))


def tied_offsets(expect, c0, search):
    """the total shifts inside the search window that a 4-periodic frame cannot tell from `expect`"""
    return {(c0[0] + oy, c0[1] + ox) for oy in range(-search, search + 1) for ox in range(-search, search + 1)
            if (c0[0] + oy - expect[0]) % 4 == 0 and (c0[1] + ox - expect[1]) % 4 == 0}


def score_map(t, r_crop, m, c0, search):
    """{(dy, dx): NCC} over the search window, the oracle's clamping and its ncc"""
    H, W = t.shape
    ys, xs = np.arange(m, H - m), np.arange(m, W - m)
    return {(c0[0] + oy, c0[1] + ox): R.ncc(t[np.ix_(np.clip(ys + c0[0] + oy, 0, H - 1), np.clip(xs + c0[1] + ox, 0, W - 1))].astype(np.float64),
                                            r_crop)
            for oy in range(-search, search + 1) for ox in range(-search, search + 1)}


def score_map_padded(t, r_crop, m, c0, search):
    """the same map with the frame extended by np.pad(mode='edge') instead of clamped indices"""
    H, W = t.shape
    p = max(abs(c0[0]), abs(c0[1])) + search
    tp = np.pad(t.astype(np.float64), p, mode="edge")
    return {(c0[0] + oy, c0[1] + ox): R.ncc(tp[p + m + c0[0] + oy:p + H - m + c0[0] + oy, p + m + c0[1] + ox:p + W - m + c0[1] + ox], r_crop)
            for oy in range(-search, search + 1) for ox in range(-search, search + 1)}


def brute_argmax(smap):
    """the header's tie rule by sorted() over every offset: the largest score, then |dy| + |dx|, then dy, then dx"""
    return sorted((-s, abs(dy) + abs(dx), dy, dx) for (dy, dx), s in smap.items())[0][2:]


# ---- 1c. init ---------------------------------------------------------------------------------------------------------------------------
HALVES = [[0.0, 0.0], [0.5, -0.5], [1.5, -1.5], [2.5, -2.5], [-3.5, 3.5], [0.49999999999999994, 0.5000000000000001]]
HALVES_EXPECT = [[0, 0], [0, 0], [2, -2], [2, -2], [-4, 4], [0, 1]]
HALVES_REF3_EXPECT = [[-2, 2], [-2, 2], [-1, 1], [0, 0], [-6, 6], [-2, 3]]
OUTSIDE_SHIFTS = [(0.0, 0.0), (7.3, -6.2), (-6.6, 5.4)]
HUGE_INIT = [[0.0, 0.0], [1e6, -1e6], [-1e6, 1e6]]
HUGE_EXPECT = [[0.0, 0.0], [999998.0, -999998.0], [-999998.0, 999998.0]]
REFUSED_INITS = {"past_1e6": [[0.0, 0.0], [np.nextafter(1e6, np.inf), 0.0], [0.0, 0.0]], "nan": [[0.0, 0.0], [0.0, np.nan], [0.0, 0.0]],
                 "past_minus_1e6": [[0.0, 0.0], [0.0, 0.0], [0.0, -np.nextafter(1e6, np.inf)]]}

# ---- 2. refinement ----------------------------------------------------------------------------------------------------------------------
REFINE_SHIFTS = [(0.0, 0.0), (1.4, -1.4), (0.3, -0.2)]
REFINE_KW = dict(search=0, border=4)
# (n_iter, tol) -> frame 1 exactly (or None: the oracle), status of frames 1 and 2
REFINE_ROWS = [(1, 1e-4, (0.5, -0.5), (3, 3)), (2, 1e-4, (1.0, -1.0), (3, 3)), (3, 0.0, None, (3, 3)), (10, 1e-4, None, (0, 0)),
               (10, 1.0, (0.5, -0.5), (0, 0)), (0, 1e-4, (0.0, 0.0), (0, 0))]


@functools.lru_cache(maxsize=None)
def refine_frames():
    """96 x 112: a smooth scene, the scene shifted by (1.4, -1.4) and by (0.3, -0.2).  Seed and smoothing are chosen so that the oracle's
    first step below tol = 1e-4 is more than ten times below it for both frames (asserted by the host test)"""
    return frames_of(96, 112, REFINE_SHIFTS, 176, sigma=2.5)


SUB3 = [(0.0, 0.0), (0.37, -0.21), (-0.44, 0.29)]  # the sub-pixel true shifts of the three-frame regime cases

# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
BATCHES = (255, 256, 512)
BATCH_N, BATCH_HW = 5, 64
BATCH_REGIME = {255: (32, 1), 256: (64, 1), 512: (256, 8)}
NOMINAL_5 = [(0.0, 0.0), (0.5, -0.5), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)]  # sr_mi355x.synth.NOMINAL_5: the patch-wise path's table
BATCH_KW = dict(init=NOMINAL_5)  # search 2, border 8: the defaults
LIMIT_B, LIMIT_KW = 65535, dict(search=0, border=0)


def prefilter_regime(B, Hc, Wc):
    """(chunk, seg) of prefilter2d (csrc/srx_prims.hpp) for a [B, Hc, Wc] stack, as tests/prims_edge_cases.py restates it"""
    chunk, seg = 256, 8
    while chunk > 32 and cdiv(Wc, 64) * cdiv(Hc, chunk) * B < 4096:
        chunk //= 2
    while seg > 1 and cdiv(Hc, 64) * cdiv(cdiv(Wc, 64), seg) * B < 4096:
        seg //= 2
    return chunk, seg


def batch_checked(B):
    """the items of a batch that are compared with the oracle: 0..7, the last 8 and every 64th"""
    return sorted(set(range(8)) | set(range(B - 8, B)) | set(range(0, B, 64)))


def batch_singles(B):
    """the items of a batch that are compared, bit for bit, with a B = 1 call"""
    return (0, 1, B // 2, B - 1)


@functools.lru_cache(maxsize=None)
def batch_item(i):
    """item i of every batch: its own scene and its own table nominal + uniform(-0.2, 0.2) -> uint8 [5, 64, 64] (read-only)"""
    tr = np.asarray(NOMINAL_5) + np.random.default_rng([SEED, 3, i]).uniform(-0.2, 0.2, (BATCH_N, 2))
    fr = frames_of(BATCH_HW, BATCH_HW, tr, 1000 + i)
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def batch_frames(B):
    fr = np.stack([batch_item(i) for i in range(B)])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def batch_oracle(i):
    return R.register_item(batch_item(i).astype(np.float64), **BATCH_KW)


@functools.lru_cache(maxsize=None)
def limit_items():
    """sixteen distinct items of two 20 x 20 frames (crop 16 x 16 at search 0, border 0) -> uint8 [16, 2, 20, 20]"""
    fr = np.stack([frames_of(20, 20, [(0.0, 0.0), (0.1 + 0.04 * i, 0.3 - 0.05 * i)], 2000 + i, sigma=1.5) for i in range(16)])
    fr.setflags(write=False)
    return fr


# ---- the single-item cases --------------------------------------------------------------------------------------------------------------
def _regime(crop, search, shifts=SUB3, seed=0, **kw):
    m = R.margin(0, search)
    return frames_of(crop[0] + 2 * m, crop[1] + 2 * m, shifts, seed), dict(search=search, border=0, **kw)


def _n32_shifts():
    sh = np.random.default_rng([SEED, 32]).uniform(-2.4, 2.4, (32, 2))
    sh[0] = 0.0
    sh[31] = (2.3, -1.6)
    return sh


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (frames uint8 [N, H, W] (read-only), keyword arguments of the call)"""
    base = tie_base()
    if name in ("ties", "ties_refined"):
        fr, kw = np.stack([base] + [np.roll(base, r, (0, 1)) for r in TIE_ROLLS]), dict(TIE_KW, n_iter=0 if name == "ties" else 10)
    elif name == "ties_total_shift":
        fr, kw = np.stack([base] + [np.roll(base, r, (0, 1)) for r in TIE2_ROLLS]), dict(TIE2_KW, n_iter=0)
    elif name.startswith("chunk_"):  # chunk_<crop width>_s<search>: crop 33 x {63, 64, 65}
        w, s = int(name.split("_")[1]), int(name[-1])
        fr, kw = _regime((33, w), s, seed=10 + w, n_iter=0)
    elif name == "crop16_s4":
        fr, kw = _regime((16, 16), 4, seed=20, n_iter=0)
    elif name == "crop17x16_s2":
        fr, kw = _regime((17, 16), 2, seed=21, n_iter=0)
    elif name == "two_row_chunks":  # frame 160 x 2200, N = 2
        fr, kw = _regime((152, 2192), 2, shifts=SUB3[:2], seed=22, n_iter=0)
    elif name in ("halves", "halves_ref3"):
        one = frames_of(40, 40, [(0.0, 0.0)], 30)[0]
        init = np.asarray(HALVES) + (1.0 if name == "halves_ref3" else 0.0)
        fr, kw = np.stack([one] * 6), dict(search=0, border=0, n_iter=0, init=init.tolist(), ref=3 if name == "halves_ref3" else 0)
    elif name in ("outside_n0", "outside_n10"):
        fr, kw = frames_of(96, 120, OUTSIDE_SHIFTS, 31), dict(search=2, border=0, n_iter=int(name[9:]), init=[list(s) for s in OUTSIDE_SHIFTS])
    elif name in ("huge_init", "huge_init_n0"):
        fr, kw = frames_of(48, 56, SUB3, 32), dict(search=2, border=2, init=HUGE_INIT, n_iter=10 if name == "huge_init" else 0)
    elif name == "flat_reference":
        fr = frames_of(64, 72, SUB3, 33)
        fr[0] = 77
        kw = dict(n_iter=0)
    elif name == "flat_moving":
        fr = frames_of(64, 72, SUB3, 33)
        fr[1] = 77
        kw = dict()
    elif name.startswith("refine_"):  # refine_<row of REFINE_ROWS>
        n_iter, tol = REFINE_ROWS[int(name[7:])][:2]
        fr, kw = refine_frames(), dict(REFINE_KW, n_iter=n_iter, tol=tol)
    elif name == "singular_on_boundary":
        col = frames_of(96, 112, [(0.0, 0.0)], 40)[0][:, :1]
        stripes = np.tile(col, (1, 112))  # constant along x: no x information
        fr, kw = np.stack([stripes, np.roll(stripes, 2, axis=0)]), dict(search=2)
    elif name == "boundary_not_converged":
        fr, kw = frames_of(96, 112, [(0.0, 0.0), (2.3, 0.0)], 41, sigma=3.0), dict(search=2, n_iter=1)
    elif name.startswith("strip_"):  # crops 41 x {255, 256, 257}
        w = int(name[6:])
        fr, kw = frames_of(49, w + 8, SUB3, 50 + w), dict(search=1, border=1)
    elif name == "n2":
        fr, kw = frames_of(48, 56, SUB3[:2], 60), dict(search=1, border=4)
    elif name in ("n32", "n32_ref_last"):
        sh = _n32_shifts()
        ref = 31 if name == "n32_ref_last" else 0
        fr, kw = frames_of(48, 56, sh, 61), dict(search=1, border=4, n_iter=8, init=np.rint(sh).tolist(), ref=ref)
    elif name.startswith("b3_item"):  # B = 3, N = 3, ref = 1: the items of one call
        i = int(name[7:])
        fr, kw = frames_of(48, 56, np.asarray(SUB3) * (1.0 + 0.15 * i), 70 + i), dict(search=2, border=4, ref=1)
    else:
        raise KeyError(name)
    fr = u8(fr)
    fr.setflags(write=False)
    return fr, kw


CHUNK_CASES = [f"chunk_{w}_s{s}" for w in (63, 64, 65) for s in (0, 4)]
COARSE_REGIME_CASES = CHUNK_CASES + ["crop16_s4", "crop17x16_s2", "two_row_chunks"]
STRIP_CASES = ["strip_255", "strip_256", "strip_257"]
B3_CASES = ["b3_item0", "b3_item1", "b3_item2"]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """R.register_item on the case -> (d [N, 2], score [N], status [N], d_coarse [N, 2]), read-only"""
    fr, kw = case(name)
    out = R.register_item(fr.astype(np.float64), **kw)
    for a in out:
        a.setflags(write=False)
    return out


# ---- the oracle's step sequence ---------------------------------------------------------------------------------------------------------
def clamped_steps(name, n):
    """the steps the oracle takes on the case's frames, from register_item at n_iter = 0..n with tol = 0: [n, N, 2]"""
    fr, kw = case(name)
    kw = dict(kw, tol=0.0)
    d = [R.register_item(fr.astype(np.float64), **dict(kw, n_iter=i))[0] for i in range(n + 1)]
    return np.diff(np.stack(d), axis=0)


def raw_step(fr, k, d, ref=0, search=2, border=8):
    """the unclamped Gauss-Newton step of frame k at shift d, built on R.sample: -A^-1 g"""
    fr = np.asarray(fr, np.float64)
    N, H, W = fr.shape
    m = R.margin(border, search)
    w, gy, gx = R.sample(R.coefficients(fr[k]), H, W, m, np.asarray(d, np.float64))
    e = w - fr[ref][m:H - m, m:W - m]
    A = np.array([[(gy * gy).sum(), (gy * gx).sum()], [(gy * gx).sum(), (gx * gx).sum()]])
    return -np.linalg.solve(A, np.array([(gy * e).sum(), (gx * e).sum()]))
