"""Device registration (srx_register_*, sr_mi355x.register.estimate_shifts) against the independent float64 oracle of
tests/register_oracle.py: integer offsets, sub-pixel shifts, scores and status codes at x2 and x4, odd shapes, the smallest crop, batches,
determinism, the exact workspace, and what the estimates buy a reconstruction."""
import ctypes

import numpy as np
import pytest
import torch

import register_oracle as R
from oracle import sr_oracle as O
from sr_mi355x import _lib, api, synth
from sr_mi355x import register as G

pytestmark = pytest.mark.gpu

# float64: the oracle's own precision (differences are summation order); float32: the frames and the spline coefficients in float32
TOL = {"f64": 1e-8, "f32": 1e-3}


def sensor(truth, shifts, f=2, psf=None, seed=1):
    psf = synth.gaussian_psf() if psf is None else psf
    lr = np.stack([O.forward_model(truth, psf, s, f) for s in shifts])
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(lr + rng.normal(0.0, 1.0, lr.shape)), 0, 255)


def jittered(seed=5):
    nom = np.asarray(synth.NOMINAL_4)
    return nom, nom + np.random.default_rng(seed).uniform(-0.2, 0.2, nom.shape)


def oracle(frames, **kw):
    return R.register_item(frames, **kw)


def device(frames, prec, **kw):
    return G.estimate_shifts(frames, precision=prec, full=True, **kw)


def check_vs_oracle(frames, prec, **kw):
    d_o, s_o, st_o, dc_o = oracle(frames, **kw)
    init = kw.get("init")
    anchor = np.zeros(2) if init is None else np.asarray(init, np.float64)[kw.get("ref", 0)]
    d, s, st = device(frames, prec, **kw)
    d = d - anchor
    ok = st_o != 1
    assert np.array_equal(st, st_o), (st, st_o)
    assert np.abs(d - d_o).max() <= TOL[prec], (d, d_o)
    assert np.abs(s - s_o).max() <= (1e-10 if prec == "f64" else 1e-4), (s, s_o)
    # the integer stage: the coarse shift is what every frame started from (and what singular frames keep)
    assert np.array_equal(np.rint(d_o[~ok]), np.rint(d[~ok]))
    return d, d_o


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_x2_measured_vs_oracle_and_truth(prec):
    sh = np.asarray(synth.MEASURED_4)
    fr = sensor(synth.truth_image(256, 256), sh)
    d, d_o = check_vs_oracle(fr, prec, init=sh)
    assert np.abs(d - (sh - sh[0])).max() < 0.05


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_x2_jittered_ref2_vs_oracle(prec):
    nom, tr = jittered()
    fr = sensor(synth.truth_image(256, 320, seed=3), tr)
    check_vs_oracle(fr, prec, init=nom, ref=2, search=3, border=4)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_odd_shape_vs_oracle(prec):
    sh = np.asarray(synth.NOMINAL_5)
    fr = sensor(synth.truth_image(300, 554, seed=7), sh)[:, :150, :277]
    check_vs_oracle(fr, prec, init=sh, search=1, border=3, n_iter=6)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_smallest_crop_vs_oracle(prec):
    # crop exactly 16 x 16: H = 16 + 2 (border + search + 2)
    search, border = 2, 1
    n = 16 + 2 * (border + search + 2)
    sh = np.asarray(synth.MEASURED_4)
    fr = sensor(synth.truth_image(2 * n, 2 * n, seed=9), sh)
    check_vs_oracle(fr, prec, init=sh, search=search, border=border)
    with pytest.raises(ValueError):
        G.estimate_shifts(fr[:, :n - 1], init=sh, search=search, border=border)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_x4_phases_vs_oracle(prec):
    sh = np.asarray(synth.phase_shifts(4))
    fr = sensor(synth.truth_image(256, 256, seed=4), sh, f=4)
    check_vs_oracle(fr, prec, init=sh, search=1, border=2, n_iter=8)


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_batch_is_bit_identical_to_single_items_and_runs(prec):
    nom, tr = jittered()
    items = [sensor(synth.truth_image(192, 224, seed=s), tr + 0.05 * s, seed=s) for s in range(3)]
    batch = torch.from_numpy(np.stack(items)).cuda()
    d, s, st = G.estimate_shifts(batch, init=nom, precision=prec, full=True)
    d2, s2, st2 = G.estimate_shifts(batch, init=nom, precision=prec, full=True)
    assert d.shape == (3, 4, 2) and s.shape == (3, 4) and st.shape == (3, 4)
    assert np.array_equal(d, d2) and np.array_equal(s, s2) and np.array_equal(st, st2)
    for b in range(3):
        d1, s1, st1 = G.estimate_shifts(items[b], init=nom, precision=prec, full=True)
        assert np.array_equal(d[b], d1) and np.array_equal(s[b], s1) and np.array_equal(st[b], st1)


def test_reference_row_is_exact_and_anchor_added():
    sh = np.asarray(synth.MEASURED_4)
    fr = sensor(synth.truth_image(192, 192), sh)
    d, s, st = G.estimate_shifts(fr, ref=1, init=sh, full=True)
    assert np.array_equal(d[1], sh[1]) and s[1] == 1.0 and st[1] == 0
    d0 = G.estimate_shifts(fr, ref=1, init=sh, anchor=(0.0, 0.0))
    assert np.array_equal(d0[1], [0.0, 0.0])
    assert np.array_equal(d, d0 + sh[1])


@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_status_singular_and_boundary(prec):
    base = sensor(synth.truth_image(192, 192), [(0.0, 0.0)])[0]
    flat = np.full_like(base, 77.0)
    stripes = np.tile(base[:, :1], (1, base.shape[1]))  # constant along x: no x information
    far = np.roll(base, (3, -1), axis=(0, 1))           # 3 px: beyond search 2, on its boundary
    fr = np.stack([base, flat, stripes, far])
    d, s, st = device(fr, prec, search=2)
    d_o, s_o, st_o, _ = oracle(fr, search=2)
    assert list(st) == [0, 1, 1, 2] and np.array_equal(st, st_o)
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(s))
    assert np.array_equal(d[1], [0.0, 0.0])  # the coarse shift, kept
    assert np.abs(d - d_o).max() <= TOL[prec]
    # a shift within the search comes out exactly
    d, _, st = device(np.stack([base, np.roll(base, (2, -1), axis=(0, 1))]), prec, search=3)
    assert st[1] == 0 and np.abs(d[1] - (2.0, -1.0)).max() < 1e-3


def test_exact_workspace():
    fr = torch.from_numpy(sensor(synth.truth_image(96, 128), synth.MEASURED_4)).cuda().float()
    lib = _lib.load()
    B, N, H, W = 1, 4, 48, 64
    shifts = torch.empty((B, N, 2), dtype=torch.float64, device="cuda")
    for search in (0, 2, 4):
        need = lib.srx_register_workspace_bytes(4, B, N, H, W, search)
        for border, want in ((0, _lib.OK), (2, _lib.OK)):
            for nb, rc in ((need, want), (need - 1, _lib.E_WORKSPACE)):
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
                got = lib.srx_register_f32(api._p(fr), B, N, H, W, 0, None, search, border, 3, 1e-4, api._p(shifts), None, None,
                                           api._p(ws), ctypes.c_size_t(nb), api._stream())
                assert got == rc, (search, border, nb, got)
    torch.cuda.synchronize()
    assert np.all(np.isfinite(shifts.cpu().numpy()))


def test_c_abi_errors():
    lib = _lib.load()
    fr = torch.zeros((1, 4, 40, 40), dtype=torch.float32, device="cuda")
    out = torch.empty((1, 4, 2), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.srx_register_workspace_bytes(4, 1, 4, 40, 40, 4), dtype=torch.uint8, device="cuda")
    wp, wn = api._p(ws), ctypes.c_size_t(ws.numel())

    def call(**kw):
        a = dict(frames=api._p(fr), B=1, N=4, H=40, W=40, ref=0, search=2, border=2, n_iter=3, tol=1e-4, shifts=api._p(out))
        a.update(kw)
        return lib.srx_register_f32(a["frames"], a["B"], a["N"], a["H"], a["W"], a["ref"], None, a["search"], a["border"], a["n_iter"],
                                    a["tol"], a["shifts"], None, None, wp, wn, api._stream())

    assert call() == _lib.OK
    for kw in (dict(frames=None), dict(shifts=None), dict(ref=4), dict(ref=-1), dict(search=5), dict(search=-1), dict(n_iter=-1),
               dict(tol=float("nan")), dict(border=-1)):
        assert call(**kw) == _lib.E_INVALID, kw
    assert call(border=8) == _lib.OK  # crop 40 - 2 (8 + 2 + 2) = 16
    assert call(border=9) == _lib.E_UNSUPPORTED
    assert lib.srx_register_workspace_bytes(4, 1, 33, 40, 40, 2) > 0
    assert call(N=33, B=1) == _lib.E_UNSUPPORTED


def test_ibp_with_estimated_shifts():
    """x2, jittered nominal table: ibp with the estimates within 0.05 dB of ibp with the true shifts, and >= 0.3 dB above the table"""
    nom, tr = jittered()
    truth = synth.truth_image(512, 512)
    psf = synth.gaussian_psf()
    lr = sensor(truth, tr)
    est = G.estimate_shifts(lr, init=nom, precision="f64")
    assert np.abs((est - est[0]) - (tr - tr[0])).max() < 0.05

    def psnr(sh):
        saa = api.shift_and_add(list(lr), sh, 2)
        hr, _ = api.ibp(list(lr), sh, psf, saa, 2, 50, 0.5, verbose=False)
        b = 16
        return synth.psnr(hr[b:-b, b:-b], truth[b:-b, b:-b])

    # the reference frame's own shift is the anchor: the true one for the estimate, as for the true table
    est_anchored = G.estimate_shifts(lr, init=nom, anchor=tr[0], precision="f64")
    p_nom, p_est, p_true = psnr(nom), psnr(est_anchored), psnr(tr)
    assert abs(p_est - p_true) < 0.05, (p_nom, p_est, p_true)
    assert p_est > p_nom + 0.3, (p_nom, p_est, p_true)
