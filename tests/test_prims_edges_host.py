"""Pins the CPU oracle to SciPy at the edges tests/test_gpu_prims_edges.py tests the HIP primitives at (tests/prims_edge_cases.py):
oracle.sr_oracle.ndi_shift / ndi_zoom / blur / forward_model / back_project against scipy.ndimage.shift(order=3, mode='nearest'),
scipy.ndimage.zoom(order=3), scipy.signal.fftconvolve(mode='same') and the reference's compositions of them
(mono_cal_target/run_sr.py:157-178).  tests/test_oracle_golden.py knows the golden shapes only.

Tolerance 1e-11 DN on 0..255 data: 25 times the largest difference seen over the line-length cross (4.0e-13, scipy 1.15.3), and a
hundredth of the float64 bound the GPU tests then hold the library to.  No GPU."""
import numpy as np
import pytest

pytest.importorskip("scipy")
from scipy import ndimage  # noqa: E402
from scipy.signal import fftconvolve  # noqa: E402

import prims_edge_cases as C  # noqa: E402
from oracle import sr_oracle as O  # noqa: E402

TOL = 1e-11
KINDS = ("int", "frac")


def sp_shift(x, s):
    return ndimage.shift(x, s, order=3, mode="nearest")


def sp_zoom(x, f):
    return ndimage.zoom(x, f, order=3)


def sp_forward(hr, k, s, f):
    """run_sr.py:161-165"""
    return sp_shift(fftconvolve(hr, k, mode="same"), (s[0] * f, s[1] * f))[::f, ::f]


def sp_back(err, k, s, f, hr_shape):
    """run_sr.py:168-178"""
    up = np.zeros((err.shape[0] * f, err.shape[1] * f))
    up[::f, ::f] = err
    up = up[:hr_shape[0], :hr_shape[1]]
    up = np.pad(up, ((0, hr_shape[0] - up.shape[0]), (0, hr_shape[1] - up.shape[1])))
    return fftconvolve(sp_shift(up, (-s[0] * f, -s[1] * f)), k[::-1, ::-1], mode="same")


def run(cases):
    """cases: (label, oracle's array, SciPy's array).  Every case is compared; the failures are reported together."""
    bad, top = [], 0.0
    for label, got, want in cases:
        d, at = C.worst(got, want)
        top = max(top, d)
        if not d <= TOL:
            bad.append(f"{label}: max |oracle - scipy| = {d:.3e} at row {at[0]}, column {at[1]}")
    print(f"largest |oracle - scipy| = {top:.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("op", ["shift", "zoom"])
def test_oracle_on_the_line_length_cross(op, axis):
    def cases():
        for shape in C.cross_shapes(axis):
            for kind in KINDS:
                x = C.image(shape, kind)
                for arg in (C.CROSS_SHIFTS if op == "shift" else C.CROSS_ZOOMS):
                    yield f"{op} {arg} on {shape} ({kind})", C.ref(op, shape, arg, kind), (sp_shift if op == "shift" else sp_zoom)(x, arg)
    run(cases())


def test_oracle_on_shift_and_zoom_extremes():
    def cases():
        for shape in C.EXTREME_IMAGES:
            for kind in KINDS:
                x = C.image(shape, kind)
                for s in C.extreme_shifts(*shape):
                    yield f"shift {s} on {shape} ({kind})", C.ref("shift", shape, s, kind), sp_shift(x, s)
                for f in C.EXTREME_ZOOMS:
                    yield f"zoom {f} on {shape} ({kind})", C.ref("zoom", shape, f, kind), sp_zoom(x, f)
    run(cases())


def test_oracle_on_blur_edges():
    def cases():
        for shape in C.BLUR_IMAGES:
            for kk in C.BLUR_KERNELS:
                for kind in KINDS:
                    want = fftconvolve(C.image(shape, kind), C.blur_kernel(*kk), mode="same")
                    yield f"blur {kk} on {shape} ({kind})", C.ref("blur", shape, kk, kind), want
    run(cases())


def test_oracle_on_forward_and_back_projection():
    k = C.fb_psf()

    def cases():
        for H, W, f, s in C.fb_cases():
            for kind in KINDS:
                yield (f"forward_model f={f} shift {s} on {(H, W)} ({kind})", C.ref("forward", (H, W), (f, s), kind),
                       sp_forward(C.image((H, W), kind), k, s, f))
                for rows in C.FB_ERR_ROWS:
                    err = C.back_err((H, W), (f, s, rows), kind)
                    yield (f"back_project f={f} shift {s} err {err.shape} -> {(H, W)} ({kind})", C.ref("back", (H, W), (f, s, rows), kind),
                           sp_back(err, k, s, f, (H, W)))
    run(cases())


@pytest.mark.parametrize("case", sorted(C.BATCH_CASES))
def test_oracle_on_batch_items(case):
    """A few items of every batched case (the GPU tests compare about a hundred of them with the oracle)"""
    op, arg = C.BATCH_CASES[case][:2]

    def cases():
        for kind in KINDS:
            x = C.batch_input(case, kind)
            for i in (0, 15, 999, 2047):
                yield f"{case} item {i} ({kind})", C.batch_ref(case, kind, i, x[i]), (sp_shift if op == "shift" else sp_zoom)(x[i], arg)
    run(cases())


def test_the_batches_reach_the_regimes_they_are_there_for():
    """The heuristic of prefilter2d, restated in prims_edge_cases.prefilter_regime: chunk 64 / 128 / 256 and seg 2 / 4 / 8 on lines of several
    chunks / tiles, while a single image of the same shape stays at chunk 32, seg 1"""
    for case, (op, _, (h, w), regime) in C.BATCH_CASES.items():
        Hc, Wc = (h + 24, w + 24) if op == "shift" else (h, w)
        assert min(Hc, Wc) < 64  # float32 stays on the line kernels
        assert C.prefilter_regime(1, Hc, Wc) == (32, 1)
        got = [C.prefilter_regime(B, Hc, Wc)[0 if regime == "chunk" else 1] for B in C.BATCHES]
        assert got == ([64, 128, 256] if regime == "chunk" else [2, 4, 8]), (case, got)
        assert (Hc > 256) if regime == "chunk" else (C.cdiv(Wc, 64) > 8)
