"""Cases, inputs and reference runs shared by tests/test_ibp_offdefaults_host.py (no GPU) and tests/test_gpu_ibp_offdefaults.py.

Everything the rest of the suite holds fixed is moved here: step is 0.3 or 1.0 (never 0.5), N is 15 ... 32, the start image is random,
and the frames are chosen so that clip(.., 0, 255) acts: rough() gives 8-bit integer frames of near-black and near-white samples, and a
start image a fifth of which already sits on a bound.  The reference is oracle.sr_oracle.ibp (float64) everywhere; the value before the
last clip, which the clip test needs, is the last iteration redone with the oracle's own forward_model / back_project and is checked to
clip to the oracle's result bit for bit.

A count here is what the kernels' count plane C holds: the number of frames whose sample lands on one HR pixel.  With integer HR
shifts n_k = f s_k, frame k covers the pixels g = f i - n_k, so frames share pixels when their n_k agree modulo f -- at f = 2 the four
+-0.5 corners of NOMINAL_5 all land on the odd / odd pixels.  far_field_planes() restates that in numpy.
"""
import functools

import numpy as np

from oracle import sr_oracle as O
from sr_mi355x import _lib, synth

SEED = 11
STEPS = (0.3, 1.0)
N_ITER = 4
EB = {"f32": 4, "f64": 8}
CLIP_EXCEPTIONS = 0.005  # share of the clipped pixels that may miss the bound, all of them within the tolerance of it

N5, P4, P2 = synth.NOMINAL_5, synth.phase_shifts(4), synth.phase_shifts(2)
_rng3 = np.random.default_rng(3)
FREE = [(float(_rng3.uniform(-1.9, 1.9)), float(_rng3.uniform(-1.9, 1.9))) for _ in range(32)]
AUTO, TILES = _lib.FLAG_AUTO, _lib.FLAG_TILES
COLS, WIDE, TWO = _lib.FLAG_DIAG_COLUMN_TILES, _lib.FLAG_DIAG_WIDE_WINDOWS, _lib.FLAG_DIAG_TWO_LAUNCH


def _scaled(a, table):
    return [(a * y, a * x) for y, x in table]


def _case(f, shifts, hw, f32, f64, asym32, asym64):
    """f32: [(flags, route)] with the default route first; f64, asym32, asym64: the default route of float64 and of the 7 x 7 PSF"""
    return {"f": f, "shifts": [(float(y), float(x)) for y, x in shifts], "hw": hw,
            "routes": {"f32": f32, "f64": [(AUTO, f64)]}, "asym": {"f32": asym32, "f64": asym64}}


_Z32 = [(AUTO, "ztile"), (COLS, "ctile"), (TILES, "mosaic")]
CASES = {
    # the packed 16-bit operand (C << 12 | M) at its limit: 15 frames on the even / even pixels, 15 on the odd / odd ones, one each on
    # the other two, so C = 15 and M = 15 * 255 = 3825 on the saturated corner
    "z_c15": _case(2, [N5[0]] * 15 + [N5[1]] * 15 + [(0.5, 0.0), (0.0, 0.5)], (64, 64), _Z32, "ctile", "ztile", "mosaic"),
    # all four corners of NOMINAL_5 share the odd / odd pixels: C = 17 and M = 4335 there, both past the packed form (float planes)
    "z_c17": _case(2, [N5[0]] * 15 + [N5[1]] * 15 + [N5[2], N5[3]], (64, 64), _Z32, "ctile", "ztile", "mosaic"),
    # C = 16 with M <= 4080 < 4096: the count alone clears cmok on integer frames
    "z_c16": _case(2, [N5[0]] * 16 + [N5[1]] * 16, (64, 64), _Z32, "ctile", "ztile", "mosaic"),
    "z_n17": _case(2, (N5 * 4)[:17], (64, 72), [(AUTO, "ztile")], "ctile", "ztile", "mosaic"),
    "p_n32": _case(4, P4 * 2, (64, 64), [(AUTO, "patch"), (WIDE, "dtile"), (TILES, "mosaic")], "stile", "patch", "mosaic"),
    "p_n17": _case(4, P4 + [P4[5]], (64, 64), [(AUTO, "patch")], "stile", "patch", "mosaic"),
    "d_n32": _case(4, P4 * 2, (64, 48), [(AUTO, "dtile"), (TWO, "atile")], "mosaic", "dtile", "mosaic"),
    "d_n20": _case(2, P2 * 5, (128, 96), [(AUTO, "dtile")], "mosaic", "dtile", "mosaic"),
    "a_n32": _case(4, P4 * 2, (40, 50), [(AUTO, "atile")], "mosaic", "mosaic", "mosaic"),
    "m_n17": _case(2, ([(0.5, 0.25), (-0.5, -0.25), (0.0, 0.75)] * 6)[:17], (24, 40), [(AUTO, "atile"), (TILES, "mosaic")], "mosaic",
                   "mosaic", "mosaic"),
    "b_n16": _case(2, FREE[:16], (16, 16), [(AUTO, "btile"), (TILES, "fused")], "fused", "btile", "fused"),
    "b_n15": _case(2, FREE[:15], (20, 33), [(AUTO, "btile")], "fused", "btile", "fused"),
    "f_n17": _case(2, FREE[:17], (20, 33), [(AUTO, "fused")], "fused", "fused", "fused"),
    "f_x3": _case(3, _scaled(0.45, FREE), (20, 24), [(AUTO, "fused")], "fused", "fused", "fused"),
    "c_far": _case(2, _scaled(2.2, FREE), (12, 14), [(AUTO, "composed")], "composed", "composed", "composed"),
}
PER_ITEM_TABLES = np.stack([np.asarray(FREE[:15]), np.asarray(FREE[15:30])])  # b_n15's shape, one table per item

PSFS = {"gauss": synth.gaussian_psf, "asym": synth.asymmetric_psf}


def rough(seed, N, h, w, f):
    """(lr [N, h, w], init [h f, w f]), float64: 8-bit frames of samples in 0..30 and 225..255 with saturated corners, and a start image
    drawn from -40..295 and clipped"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=(N, h, w))
    lr = np.rint(np.where(u < 0.5, rng.uniform(0, 30, (N, h, w)), rng.uniform(225, 255, (N, h, w))))
    lr[:, :4, :4] = 255
    lr[:, -4:, -4:] = 0
    init = np.clip(rng.uniform(-40, 295, (h * f, w * f)), 0, 255)
    return lr, init


@functools.lru_cache(maxsize=None)
def inputs(case, seed=SEED):
    c = CASES[case]
    lr, init = rough(seed, len(c["shifts"]), c["hw"][0], c["hw"][1], c["f"])
    lr.setflags(write=False), init.setflags(write=False)
    return lr, init


def path_for(prec, case, psf_name, flags=AUTO, shifts=None):
    """srx_ibp_path_for: the route the library gives this case (host arithmetic, no device)"""
    c = CASES[case]
    sh = np.ascontiguousarray(np.asarray(c["shifts"] if shifts is None else shifts, dtype=np.float64))
    k = np.ascontiguousarray(PSFS[psf_name]())
    (h, w), f = c["hw"], c["f"]
    return _lib.load().srx_ibp_path_for(EB[prec], len(sh), h, w, h * f, w * f, f, sh.ctypes.data_as(_lib._HD), k.ctypes.data_as(_lib._HD),
                                        k.shape[0], k.shape[1], flags).decode()


def oracle_ibp(lr, shifts, psf, init, f, n_iter, step):
    """oracle.sr_oracle.ibp on 8 threads -> (hr, errors)"""
    O.set_threads(8)
    try:
        hr, errs = O.ibp(list(lr), shifts, psf, init, f, n_iter, step)
    finally:
        O.set_threads(1)
    return hr, np.asarray(errs)


def oracle_run(lr, shifts, psf, init, f, n_iter, step):
    """-> (hr, errors, v): oracle.sr_oracle.ibp, and v = the state before the last clip, so that hr == clip(v, 0, 255)"""
    hr, errs = oracle_ibp(lr, shifts, psf, init, f, n_iter, step)
    O.set_threads(8)
    try:
        prev = O.ibp(list(lr), shifts, psf, init, f, n_iter - 1, step)[0] if n_iter > 1 else np.array(init, dtype=np.float64)
        corr = np.zeros_like(prev)
        for l, s in zip(lr, shifts):  # orc_ibp's last pass, frame by frame in its order
            corr += O.back_project(l - O.forward_model(prev, psf, s, f), psf, s, f, prev.shape)
        v = prev + step * corr / float(len(shifts))
    finally:
        O.set_threads(1)
    return hr, np.asarray(errs), v


@functools.lru_cache(maxsize=None)
def reference(case, psf_name, step, n_iter=N_ITER):
    """The oracle on a case's inputs, computed once per process and read-only: {"hr", "errors", "v"}"""
    c = CASES[case]
    lr, init = inputs(case)
    hr, errs, v = oracle_run(lr, c["shifts"], PSFS[psf_name](), init, c["f"], n_iter, step)
    for a in (hr, errs, v):
        a.setflags(write=False)
    return {"hr": hr, "errors": errs, "v": v}


def clip_shares(case, ref):
    """(share of pixels at 0.0, share at 255.0, share that starts strictly inside (0, 255) and ends on a bound)"""
    init = inputs(case)[1]
    hr = ref["hr"]
    on = (hr == 0.0) | (hr == 255.0)
    return float((hr == 0.0).mean()), float((hr == 255.0).mean()), float((on & (init > 0.0) & (init < 255.0)).mean())


def clip_misses(hr, ref, tol):
    """Where the oracle is exactly on a bound, `hr` must be too.  -> (clipped, near, far): the oracle's pixels on a bound; those of them
    `hr` is off the bound at while the oracle's value before the clip is within tol of it (tolerated, counted); and the other misses."""
    o, v = ref["hr"], ref["v"]
    lo, hi = o == 0.0, o == 255.0
    miss = (lo & (hr != 0.0)) | (hi & (hr != 255.0))
    near = (lo & (v > -tol)) | (hi & (v < 255.0 + tol))
    return int(lo.sum() + hi.sum()), int((miss & near).sum()), int((miss & ~near).sum())


def far_field_planes(case):
    """numpy restatement of the count and sum planes of a delta = 0 case: (C, M) [H, W] with C = the number of frames whose sample lands
    on an HR pixel, M = the sum of those samples -- frame k's sample (i, j) at g = f (i, j) - n_k, n_k = f s_k.  The first -min(n_k) rows
    and columns (the near band, where row / column 0 is replicated) travel as per-pixel lists and are left zero, as in the kernels."""
    c = CASES[case]
    f, (h, w) = c["f"], c["hw"]
    lr = inputs(case)[0]
    n = np.rint(np.asarray(c["shifts"]) * f).astype(int)
    assert np.array_equal(n, np.asarray(c["shifts"]) * f), "integer HR shifts only"
    C, M = np.zeros((h * f, w * f)), np.zeros((h * f, w * f))
    nby, nbx = max(0, -n[:, 0].min()), max(0, -n[:, 1].min())
    for k, (ny, nx) in enumerate(n):
        gy, gx = f * np.arange(h) - ny, f * np.arange(w) - nx
        my, mx = (gy >= nby) & (gy < h * f), (gx >= nbx) & (gx < w * f)
        C[np.ix_(gy[my], gx[mx])] += 1
        M[np.ix_(gy[my], gx[mx])] += lr[k][np.ix_(my, mx)]
    return C, M
