"""The users of the segmented LDS spline walk (fused::walk_pass, csrc/srx_fused.hpp) against the oracle, with the LAST tile's walk in every
regime it can be in while the interior tiles stay in theirs.

A walk over lines of n outputs (n = n_in - 3 where the FIR runs first, MODE 1) asks for NSEG threads per line and gets
    four   unless nlines > 64 or n - need_lo < 4 (R + 8), then
    two    unless ((R + 7) & ~7) > ((n - R) & ~7), then
    one thread per line,
R = 11 (float32) / 23 (float64) in the tile kernels, 20 in k_prefilter_tile: two threads from n = 27 / 47 / 44 on, four from
n - need_lo = 76 / 124 on.  regime() restates that, the *_walks functions restate each kernel's region arithmetic (its n_in, need_lo and
line count per tile), and test_case_table_reaches_every_regime -- no GPU -- holds the case table to them: every regime a kernel can reach
over the sizes a call can have is reached by a case, with n on both sides of a threshold wherever both sides exist.  What the arithmetic
says cannot happen today: four threads per line in float64 anywhere (the longest line has n - need_lo = 93 < 124), in k_saa_tile and
k_saa_shift in float32 (n - need_lo <= 75) and on the last tile of k_fwd_mosaic; more than 64 lines at a call site that asks for four;
one thread per line in float32 in k_bwd_mosaic, k_bwd_tile and k_fwd_tile (n >= 27).

Tolerances are test_gpu_parity's for the same paths (PRIM_TOL for shift_and_add, zoom and shift; IBP_TOL and ERR_RTOL for ibp), on the data
of its test_fused_path_vs_oracle (a smooth truth, the oracle's forward model, integer sensor samples).  One item, 2 iterations.
"""
import functools

import numpy as np
import pytest

from sr_mi355x import synth
from test_gpu_parity import ERR_RTOL, IBP_TOL, PRIM_TOL

TS, NPAD, WU = 64, 12, 20
R = {"f32": 11, "f64": 23}
ITERS = 2


def cdiv(a, b):
    return -(-a // b)


def regime(nseg, r, mode, nlines, n_in, need_lo=0):
    """What a walk_pass<.., MODE, R, NSEG> call runs as: "4", "2" (asked for two), "2 short" / "2 lines" (asked for four), "1" """
    n = n_in - 3 if mode == 1 else n_in
    name = str(nseg)
    if nseg == 4:
        if nlines > 64:
            nseg, name = 2, "2 lines"
        elif n - need_lo < 4 * (r + 8):
            nseg, name = 2, "2 short"
    if nseg == 2 and ((r + 7) & ~7) > ((n - r) & ~7):
        name = "1"
    return name


def first_n_for_two(r):
    return r + ((r + 7) & ~7)


# ---------------------------------------------------------------------------------------------------------------------------------
# region arithmetic: (kernel, axis, NSEG, R, MODE, nlines, n_in, need_lo) of every walk a launch makes on a [H, W] HR plane
# ---------------------------------------------------------------------------------------------------------------------------------
def tiles(H, W, step=TS):
    return [(r0, c0) for r0 in range(0, H, step) for c0 in range(0, W, step)]


def saa_walks(kernel, prec, H, W):
    """k_saa_tile (one-pass form) and k_saa_shift: the region of an output tile in the padded plane, R of halo, + 3 for the FIR"""
    r, Hp, Wp, out = R[prec], H + 2 * NPAD, W + 2 * NPAD, []
    for r0, c0 in tiles(H, W):
        pa, pb = max(0, r0 + NPAD - r), min(Hp, r0 + NPAD + TS + r)
        qa, qb = max(0, c0 + NPAD - r), min(Wp, c0 + NPAD + TS + r)
        nr, nc = pb - pa, qb - qa
        r_lo = r0 + NPAD - pa
        r_hi = min(r_lo + TS, nr)
        out += [(kernel, 0, 2, r, 1, nc + 3, nr + 3, r_lo), (kernel, 1, 4, r, 1, max(r_hi - r_lo, 0), nc + 3, c0 + NPAD - qa)]
    return out


def bwd_region(prec, H, W, r0, c0):
    r, Hp, Wp = R[prec], H + 2 * NPAD, W + 2 * NPAD
    pa, pb = max(0, r0 + 9 - r), min(Hp, r0 + TS + 15 + r)
    qa, qb = max(0, c0 + 9 - r), min(Wp, c0 + TS + 15 + r)
    return pa, qa, pb - pa, qb - qa, r0 + 9 - pa, min(r0 + TS + 15, Hp) - pa


def bwd_mosaic_walks(prec, H, W, sep):
    r, out = R[prec], []
    for r0, c0 in tiles(H, W):
        pa, qa, nr, nc, r_lo, r_hi = bwd_region(prec, H, W, r0, c0)
        out.append(("k_bwd_mosaic", 0, 2, r, 1, nc + 3, nr + 3, r_lo))
        if sep:  # the blur down leaves TS rows
            out.append(("k_bwd_mosaic", 1, 4, r, 1, TS, nc + 3, c0 + 9 - qa))
        else:
            out.append(("k_bwd_mosaic", 1, 2, r, 1, max(r_hi - r_lo, 0), nc + 3, c0 + 9 - qa))
    return out


def bwd_tile_walks(prec, H, W):
    r, out = R[prec], []
    for r0, c0 in tiles(H, W):
        pa, qa, nr, nc, r_lo, r_hi = bwd_region(prec, H, W, r0, c0)
        out += [("k_bwd_tile", 0, 2, r, 0, nc, nr, 0), ("k_bwd_tile", 1, 2, r, 0, r_hi - r_lo, nc, 0)]
    return out


def fwd_mosaic_walks(prec, H, W, shifts, f):
    """a common fraction > 0: D = 3, the near band is the first PB = 13 - min floor(f s) rows / columns of the G plane [H + 27, W + 27]"""
    r, Hp, Wp, D, out = R[prec], H + 2 * NPAD, W + 2 * NPAD, 3, []
    PBy, PBx = (13 - min(int(np.floor(s[a] * f + 1e-12)) for s in shifts) for a in (0, 1))
    for p0, q0 in tiles(Hp + 3, Wp + 3):
        pa, pb = max(0, p0 - D - r), min(Hp, p0 - D + TS + 3 + r)
        qa, qb = max(0, q0 - D - r), min(Wp, q0 - D + TS + 3 + r)
        nr, nc = pb - pa, qb - qa
        if nr > 3 and nc > 3:
            r_lo, r_hi = max(0, p0 - D - pa), min(nr - 3, p0 - D + TS - pa)
            r_lo_w, c_lo_w = 0 if p0 < PBy else r_lo, 0 if q0 < PBx else max(0, q0 - D - qa)
            out += [("k_fwd_mosaic", 0, 2, r, 2, nc, nr, r_lo_w), ("k_fwd_mosaic", 1, 4, r, 2, max(r_hi - r_lo_w, 0), nc, c_lo_w)]
    return out


def fwd_tile_walks(prec, h, w, shifts, f):
    """tiles of TS / f LR pixels; the first tap of frame k sits at floor(-f s_k) - 1 + 12 from f i"""
    r, Hp, Wp, tl, out = R[prec], h * f + 2 * NPAD, w * f + 2 * NPAD, TS // f, []
    o = [[int(np.floor(-s[a] * f)) - 1 + NPAD for s in shifts] for a in (0, 1)]
    (omin_y, omax_y), (omin_x, omax_x) = ((min(v), max(v)) for v in o)
    for i0, j0 in tiles(h, w, tl):
        i1, j1 = min(i0 + tl, h), min(j0 + tl, w)
        pa, pb = max(0, f * i0 + omin_y - r), min(Hp - 1, f * (i1 - 1) + omax_y + 3 + r)
        qa, qb = max(0, f * j0 + omin_x - r), min(Wp - 1, f * (j1 - 1) + omax_x + 3 + r)
        nr, nc = pb - pa + 1, qb - qa + 1
        out += [("k_fwd_tile", 0, 2, r, 0, nc, nr, 0), ("k_fwd_tile", 1, 2, r, 0, f * (i1 - 1) + omax_y + 4 - f * i0 - omin_y, nc, 0)]
    return out


def prefilter_tile_walks(Hc, Wc):
    out = []
    for r0, c0 in tiles(Hc, Wc):
        pa, pb, qa, qb = max(0, r0 - WU), min(Hc, r0 + TS + WU), max(0, c0 - WU), min(Wc, c0 + TS + WU)
        out += [("k_prefilter_tile", 0, 2, WU, 0, qb - qa, pb - pa, 0), ("k_prefilter_tile", 1, 2, WU, 0, min(r0 + TS, Hc) - r0, qb - qa, 0)]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the calls.  Shift sets with the common fraction one half at x2, x3, x4 (the mosaic kernels with D = 3); the measured set for the
# per-frame tile kernels (float32 at x2 runs on register windows instead: x3 there)
# ---------------------------------------------------------------------------------------------------------------------------------
HALF = {2: synth.phase_shifts(2), 3: [(1 / 6, 1 / 6), (-1 / 6, 1 / 2), (1 / 2, -1 / 6)], 4: synth.phase_shifts(4)}
USERS = ("zoom", "shift", "saa_two_pass", "saa_one_pass", "fused", "mosaic_sep", "mosaic_7x7")


def walks_of(user, prec, f, h, w):
    """every walk of the kernels the call is there for"""
    H, W = h * f, w * f
    if user == "zoom":
        return prefilter_tile_walks(h, w)
    if user == "shift":
        return prefilter_tile_walks(h + 2 * NPAD, w + 2 * NPAD)
    if user == "saa_two_pass":
        return saa_walks("k_saa_shift", prec, H, W)
    if user == "saa_one_pass":
        return saa_walks("k_saa_tile", prec, H, W)
    if user == "fused":
        return fwd_tile_walks(prec, h, w, synth.MEASURED_4, f) + bwd_tile_walks(prec, H, W)
    return fwd_mosaic_walks(prec, H, W, HALF[f], f) + bwd_mosaic_walks(prec, H, W, user == "mosaic_sep")


def factors(user, prec):
    if user in ("zoom", "shift"):
        return (1,)
    if user == "fused":
        return (3, 4) if prec == "f32" else (2, 3, 4)
    return (2, 3, 4)


def precisions(user):
    return ("f32",) if user in ("zoom", "shift") else ("f32", "f64")


def facts(walks):
    """what a set of walks shows per (kernel, axis): its regimes, and the values that sit on a threshold"""
    out = {}
    for kernel, axis, nseg, r, mode, nlines, n_in, need_lo in walks:
        if nlines <= 0:
            continue
        n = n_in - 3 if mode == 1 else n_in
        s = out.setdefault((kernel, axis), set())
        s.add(regime(nseg, r, mode, nlines, n_in, need_lo))
        if n in (first_n_for_two(r) - 1, first_n_for_two(r)):
            s.add(f"n = {n}")
        if nseg == 4 and nlines <= 64 and n - need_lo in (4 * (r + 8) - 1, 4 * (r + 8)):
            s.add(f"n - need_lo = {n - need_lo}")
    return out


def merged(list_of_facts):
    out = {}
    for d in list_of_facts:
        for k, v in d.items():
            out.setdefault(k, set()).update(v)
    return out


# (user, precision, f, LR h, LR w): HR = f h x f w, square so that one call puts the last tile of both axes at the same n.  The comment
# names what the last tile (l. t.) is there for; the interior tiles and the first one are what they are on every plane of several tiles.
CASES = [
    # k_prefilter_tile, R = 20: the last tile's region is (len mod 64) + 20 long; a shift filters the plane padded by 12 a side
    ("zoom", "f32", 1, 87, 87),            # l. t. n = 43: one thread per line
    ("zoom", "f32", 1, 88, 88),            # l. t. n = 44: two
    ("shift", "f32", 1, 127, 127),         # the padded plane is 151 long: l. t. n = 43
    ("shift", "f32", 1, 64, 64),           # 88 long: l. t. n = 44
    # k_saa_shift / k_saa_tile: n = (W mod 64) + 12 + R on the last tile; the row walk asks for four threads and never gets them
    ("saa_two_pass", "f32", 3, 65, 65),    # 195: l. t. n = 26, one thread; the interior tiles n - need_lo = 75, one short of four threads
    ("saa_two_pass", "f32", 2, 34, 34),    # 68: l. t. n = 27, two
    ("saa_two_pass", "f64", 3, 25, 25),    # 75: l. t. n = 46, one thread
    ("saa_two_pass", "f64", 2, 38, 38),    # 76: l. t. n = 47, two
    ("saa_one_pass", "f32", 3, 65, 65),
    ("saa_one_pass", "f32", 2, 34, 34),
    ("saa_one_pass", "f64", 3, 25, 25),
    ("saa_one_pass", "f64", 2, 38, 38),
    # k_fwd_tile / k_bwd_tile: two threads at most.  float32: n >= 27 on every tile
    ("fused", "f32", 3, 43, 43),           # 129: k_bwd_tile's l. t. n = 27
    ("fused", "f64", 4, 18, 18),           # 72: l. t. n = 46 in both kernels, one thread
    ("fused", "f64", 3, 24, 24),           # 72: k_fwd_tile's l. t. n = 47 (tiles of 21 LR pixels)
    ("fused", "f64", 3, 67, 67),           # 201: k_bwd_tile's l. t. n = 47
    # k_fwd_mosaic (tiles of the G plane, W + 27 wide) and k_bwd_mosaic; the separable k_bwd_mosaic asks for four threads on its row walk
    ("mosaic_sep", "f32", 2, 58, 58),      # 116: k_fwd_mosaic l. t. n = 26, its first tile n - need_lo = 75 (two), its second 4 threads;
    #                                        k_bwd_mosaic: first tile four threads, l. t. two (short for four)
    ("mosaic_sep", "f32", 3, 39, 39),      # 117: k_fwd_mosaic l. t. n = 27
    ("mosaic_sep", "f32", 3, 43, 43),      # 129: k_bwd_mosaic l. t. n = 27
    ("mosaic_sep", "f32", 2, 18, 30),      # 60 wide, one tile: k_bwd_mosaic n - need_lo = 75
    ("mosaic_sep", "f32", 3, 12, 59),      # 177 wide: k_fwd_mosaic l. t. n - need_lo = 76 (the plane ends inside the third tile's halo)
    ("mosaic_sep", "f32", 3, 12, 63),      # 189 wide: k_bwd_mosaic l. t. n - need_lo = 76
    ("mosaic_sep", "f64", 2, 30, 30),      # 60: k_fwd_mosaic l. t. n = 46
    ("mosaic_sep", "f64", 2, 36, 36),      # 72: k_bwd_mosaic l. t. n = 46
    ("mosaic_sep", "f64", 3, 63, 63),      # 189: k_fwd_mosaic l. t. n = 47
    ("mosaic_sep", "f64", 3, 67, 67),      # 201: k_bwd_mosaic l. t. n = 47
    ("mosaic_7x7", "f32", 2, 58, 58),
    ("mosaic_7x7", "f32", 3, 39, 39),
    ("mosaic_7x7", "f32", 3, 43, 43),
    ("mosaic_7x7", "f32", 3, 12, 59),
    ("mosaic_7x7", "f64", 2, 30, 30),
    ("mosaic_7x7", "f64", 2, 36, 36),
    ("mosaic_7x7", "f64", 3, 63, 63),
    ("mosaic_7x7", "f64", 3, 67, 67),
]


def case_id(c):
    return f"{c[0]}-{c[1]}-x{c[2]}-{c[3]}x{c[4]}"


@functools.lru_cache(maxsize=None)
def reachable(user, prec):
    """facts over the sizes a call can have: one axis from 32 to 330 HR samples, the other short, both ways round"""
    found = []
    for f in factors(user, prec):
        lo = 64 if f == 1 else cdiv(32, f)
        for n in range(lo, 330 // f + 1):
            for h, w in ((n, cdiv(36, f) if f > 1 else 70), (cdiv(36, f) if f > 1 else 70, n)):
                found.append(facts(walks_of(user, prec, f, h, w)))
    return merged(found)


def test_case_table_reaches_every_regime():
    """No GPU.  Per user, precision, kernel and axis: whatever any size reaches -- a regime, a value of n on a threshold -- a case reaches"""
    missing = []
    for user in USERS:
        for prec in precisions(user):
            have = merged([facts(walks_of(*c)) for c in CASES if c[0] == user and c[1] == prec])
            for key, want in sorted(reachable(user, prec).items()):
                lack = want - have.get(key, set())
                if lack:
                    missing.append(f"{user} {prec} {key[0]} axis {key[1]}: no case reaches {sorted(lack)}")
    assert not missing, "\n".join(missing)
    # the regimes themselves, from the kernels' formulas at the interior tile of a large plane and at the thresholds
    assert regime(4, 11, 1, 64, 89, 11) == "2 short" and regime(4, 11, 2, 64, 89, 11) == "4" and regime(4, 11, 1, 64, 95, 11) == "4"
    assert regime(4, 23, 1, 64, 119, 23) == "2 short" and regime(4, 11, 2, 65, 89, 11) == "2 lines"
    assert [regime(2, r, 0, 64, n) for r, n in ((11, 26), (11, 27), (23, 46), (23, 47), (20, 43), (20, 44))] == ["1", "2"] * 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the GPU side: every case against the oracle.  References are computed once per process, shared and read-only (a call gets a copy).
# ---------------------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _setup(user, f):
    """(shifts, PSF) of a user: the Gaussian takes k_bwd_mosaic to its separable branch, synth.asymmetric_psf to its 7 x 7 one"""
    shifts = synth.MEASURED_4 if user == "fused" else HALF[f]
    return shifts, synth.gaussian_psf() if user in ("mosaic_sep", "saa") else synth.asymmetric_psf()


@functools.lru_cache(maxsize=None)
def saa_scene(user, f, h, w):
    """(frames [N, h, w], the oracle's shift_and_add of them)"""
    from oracle import sr_oracle as O
    shifts, psf = _setup(user, f)
    truth = synth.truth_image(h * f, w * f, seed=77)
    lr = synth.sensor_frames(np.stack([O.forward_model(truth, psf, s, f) for s in shifts]), seed=78).astype(np.float64)
    return _frozen(lr, O.shift_and_add(list(lr), shifts, f))


@functools.lru_cache(maxsize=None)
def ibp_ref(user, f, h, w):
    from oracle import sr_oracle as O
    shifts, psf = _setup(user, f)
    lr, saa_o = saa_scene(user, f, h, w)
    hr_o, err_o = O.ibp(list(lr), shifts, psf, saa_o, f, ITERS, 0.5)
    return _frozen(hr_o, np.asarray(err_o))


@functools.lru_cache(maxsize=None)
def prim_ref(user, h, w):
    from oracle import sr_oracle as O
    x = np.rint(np.random.default_rng([459, h, w]).uniform(0, 255, (h, w)))
    return _frozen(x, O.ndi_zoom(x, 2) if user == "zoom" else O.ndi_shift(x, (0.37, -0.61)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_last_tile_in_every_regime(case):
    from sr_mi355x import _lib, api as S
    from test_gpu_parity import close
    user, prec, f, h, w = case
    if user in ("zoom", "shift"):
        x, ref = prim_ref(user, h, w)
        got = S.zoom_batched(x[None].copy(), 2, precision=prec) if user == "zoom" else S.shift_batched(x[None].copy(), (0.37, -0.61), precision=prec)
        close(got[0].cpu().numpy(), ref, PRIM_TOL[prec])
        return
    if user.startswith("saa"):
        lr, saa_o = saa_scene("saa", f, h, w)
        got = S.shift_and_add_batched(lr[None].copy(), HALF[f], f, precision=prec, flags=_lib.FLAG_DIAG_SAA_ONE_PASS if user == "saa_one_pass" else 0)
        assert S.last_path() == "mosaic"
        close(got[0].cpu().numpy(), saa_o, PRIM_TOL[prec])
        return
    shifts, psf = _setup(user, f)
    (lr, saa_o), (hr_o, err_o) = saa_scene(user, f, h, w), ibp_ref(user, f, h, w)
    hr, errs = S.ibp_batched(lr[None].copy(), shifts, psf, saa_o[None].copy(), f, ITERS, 0.5, precision=prec,
                             flags=_lib.FLAG_PER_FRAME if user == "fused" else _lib.FLAG_TILES)
    assert S.last_path() == ("fused" if user == "fused" else "mosaic")
    close(hr[0].cpu().numpy(), hr_o, IBP_TOL[prec])
    np.testing.assert_allclose(errs[0].cpu().numpy(), err_o, rtol=ERR_RTOL[prec])
