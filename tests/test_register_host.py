"""Registration without a GPU: the oracle of tests/register_oracle.py against the truth on synthetic x2 sessions (the accuracy the device
is held to by tests/test_gpu_register.py), its sign convention, ref != 0 and the anchor of sr_mi355x.register.estimate_shifts, the
workspace formula of srx_register_workspace_bytes, and the wrapper's argument errors (raised before any device work)."""
import numpy as np
import pytest

import register_oracle as R
from oracle import sr_oracle as O
from sr_mi355x import _lib, synth
from sr_mi355x import register as G

ndi = pytest.importorskip("scipy.ndimage")

# what the oracle achieves on these scenes (max error over the frames, LR px): MEASURED_4 0.0142, jittered nominal 0.0153 -- held with a
# margin of about 1.5x
BOUND_MEASURED, BOUND_JITTER = 0.02, 0.025


def sensor(truth, shifts, f=2, seed=1):
    lr = np.stack([O.forward_model(truth, synth.gaussian_psf(), s, f) for s in shifts])
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(lr + rng.normal(0.0, 1.0, lr.shape)), 0, 255)


@pytest.fixture(scope="module")
def truth():
    return synth.truth_image(512, 512)


def test_oracle_accuracy_measured(truth):
    sh = np.asarray(synth.MEASURED_4)
    d, score, st, _ = R.register_item(sensor(truth, sh), ref=0, init=sh)
    assert list(st) == [0, 0, 0, 0]
    assert np.abs(d - (sh - sh[0])).max() < BOUND_MEASURED
    assert np.all(score[1:] > 0.99) and score[0] == 1.0


def test_oracle_accuracy_jittered_nominal(truth):
    nom = np.asarray(synth.NOMINAL_4)
    tr = nom + np.random.default_rng(5).uniform(-0.2, 0.2, nom.shape)
    d, _, st, dc = R.register_item(sensor(truth, tr), ref=0, init=nom)
    assert list(st) == [0, 0, 0, 0]
    assert np.abs(d - (tr - tr[0])).max() < BOUND_JITTER
    # the table alone is up to 0.4 px off; the coarse stage lands on the nearest integer
    assert np.abs((nom - nom[0]) - (tr - tr[0])).max() > 0.2
    assert np.abs(dc - (tr - tr[0])).max() <= 0.5 + 0.4


def test_sign_convention():
    """frames[k] = ndi.shift(frames[ref], d) -> d, with d in (dy, dx) like shifts_yx"""
    base = synth.truth_image(160, 192, seed=3)
    base = ndi.gaussian_filter(base, 1.0)
    for d in [(0.3, -0.7), (-1.25, 0.4), (2.0, 1.0)]:
        moved = ndi.shift(base, d, order=3, mode="nearest")
        est, _, st, _ = R.register_item(np.stack([base, moved]), search=3, n_iter=20)
        assert st[1] == 0 and np.abs(est[1] - d).max() < 0.01, (d, est[1])
    # and the frames of forward_model carry exactly their shifts_yx difference
    sh = [(0.0, 0.0), (0.6, -0.3)]
    est, *_ = R.register_item(sensor(synth.truth_image(256, 256), sh), init=sh)
    assert np.abs(est[1] - (0.6, -0.3)).max() < 0.03


def test_ref_not_zero(truth):
    sh = np.asarray(synth.MEASURED_4)
    fr = sensor(truth, sh)
    d0, *_ = R.register_item(fr, ref=0, init=sh)
    d2, _, st, _ = R.register_item(fr, ref=2, init=sh)
    assert np.array_equal(d2[2], [0.0, 0.0]) and st[2] == 0
    # relative to another reference the same frames keep their differences (to the estimate's accuracy)
    assert np.abs((d2 - d2[0]) - d0).max() < 2 * BOUND_MEASURED


def test_oracle_samples_like_ndi_shift():
    """the oracle's interpolant is scipy's: t(i + d) on the crop equals ndi.shift(t, -d) there"""
    t = synth.truth_image(64, 80, seed=2)
    coef = R.coefficients(t)
    for d in [(0.37, -1.6), (-0.5, 0.25), (1.0, 0.0)]:
        w, gy, gx = R.sample(coef, 64, 80, 6, np.asarray(d))
        want = ndi.shift(t, (-d[0], -d[1]), order=3, mode="nearest")[6:-6, 6:-6]
        assert np.abs(w - want).max() < 1e-9
        # the analytic gradient against a central difference of the interpolant
        h = 1e-5
        wy = (R.sample(coef, 64, 80, 6, np.asarray(d) + (h, 0))[0] - R.sample(coef, 64, 80, 6, np.asarray(d) - (h, 0))[0]) / (2 * h)
        wx = (R.sample(coef, 64, 80, 6, np.asarray(d) + (0, h))[0] - R.sample(coef, 64, 80, 6, np.asarray(d) - (0, h))[0]) / (2 * h)
        assert np.abs(gy - wy).max() < 1e-4 and np.abs(gx - wx).max() < 1e-4


def test_anchor_and_ref_in_wrapper_validation():
    """_check resolves the anchor (init[ref], else zeros) and the batch layout without a device"""
    sh = np.asarray(synth.MEASURED_4)
    B, N, H, W, batched, init, anchor = G._check((4, 64, 64), 2, sh, None, 2, 8, 10, 1e-4)
    assert (B, N, H, W, batched) == (1, 4, 64, 64, False) and np.array_equal(anchor, sh[2])
    *_, anchor = G._check((4, 64, 64), 1, None, None, 2, 8, 10, 1e-4)
    assert np.array_equal(anchor, [0.0, 0.0])
    B, N, H, W, batched, _, anchor = G._check((3, 4, 64, 64), 0, sh, (0.1, -0.2), 2, 8, 10, 1e-4)
    assert (B, N, batched) == (3, 4, True) and np.array_equal(anchor, [0.1, -0.2])


@pytest.mark.parametrize("bad", [dict(ref=4), dict(ref=-1), dict(search=5), dict(search=-1), dict(n_iter=-1), dict(tol=-1.0),
                                 dict(tol=float("nan")), dict(border=-1), dict(border=21), dict(init=np.zeros((3, 2))),
                                 dict(init=np.full((4, 2), np.nan)), dict(anchor=(1.0, 2.0, 3.0))])
def test_wrapper_argument_errors_before_device_work(bad):
    frames = [np.zeros((64, 64))] * 4
    with pytest.raises(ValueError):
        G.estimate_shifts(frames, **bad)


def test_wrapper_shape_errors():
    with pytest.raises(ValueError):
        G.estimate_shifts([np.zeros((64, 64))])  # one frame
    with pytest.raises(ValueError):
        G.estimate_shifts(np.zeros((64, 64)))
    with pytest.raises(ValueError):
        G.estimate_shifts(np.zeros((33, 64, 64)))


def test_workspace_bytes_formula():
    lib = _lib.load()
    assert lib.srx_register_workspace_bytes(4, 1, 4, 48, 64, 2) > 0
    # two padded coefficient planes per moving frame dominate; float64 frames need more
    n4 = lib.srx_register_workspace_bytes(4, 1, 5, 1536, 2048, 2)
    assert n4 >= 2 * 4 * (1536 + 24) * (2048 + 24) * 4
    assert lib.srx_register_workspace_bytes(8, 1, 5, 1536, 2048, 2) > n4
    assert lib.srx_register_workspace_bytes(4, 3, 5, 1536, 2048, 2) > 2.9 * n4
    assert G.workspace_bytes(4, 1, 5, 1536, 2048, 2) == n4
    for args in [(2, 1, 4, 64, 64, 2), (4, 0, 4, 64, 64, 2), (4, 1, 1, 64, 64, 2), (4, 1, 4, 64, 64, 5), (4, 1, 4, 64, 64, -1),
                 (4, 1, 4, 23, 64, 2)]:
        assert lib.srx_register_workspace_bytes(*args) == 0, args
    # the smallest crop: 16 + 2 (search + 2) at border 0
    assert lib.srx_register_workspace_bytes(4, 1, 4, 24, 24, 2) > 0
