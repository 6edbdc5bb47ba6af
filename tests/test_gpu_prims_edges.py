"""The HIP primitives at every regime boundary of their code: srx_shift_cubic / srx_zoom_cubic (the cubic B-spline prefilter behind them, the
tap builder), srx_blur, srx_forward / srx_backproject and the pointwise glue, against the CPU oracle (float64; pinned to SciPy on the same
cases by tests/test_prims_edges_host.py).  The cases and what each is there for: tests/prims_edge_cases.py.

Tolerances are test_gpu_parity.PRIM_TOL (f64 1e-9, f32 5e-4 DN on 0..255 data); index maps, means and batch-against-single comparisons
are bit for bit.  A test runs all its cases and then fails with one line per case that missed: the precision, the operation, the shape
and the row and column of the largest error.  Every test prints the largest error it saw (pytest -s).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import sr_mi355x as S  # noqa: E402

import prims_edge_cases as C  # noqa: E402
from oracle import sr_oracle as O  # noqa: E402
from test_gpu_parity import PRIM_TOL  # noqa: E402

NP_DT = {"f64": np.float64, "f32": np.float32}
TORCH_DT = {"f64": torch.float64, "f32": torch.float32}


@pytest.fixture(params=["f64", "f32"])
def prec(request):
    S.set_precision(request.param)
    yield request.param
    S.set_precision("f32")


class Tally:
    """Collects the cases of one test: the largest error, and a line per case that missed"""

    def __init__(self, group, prec):
        self.group, self.prec, self.bad, self.top, self.n = group, prec, [], (0.0, "-"), 0

    def close(self, what, got, want):
        tol = PRIM_TOL[self.prec]
        d, at = C.worst(got, want)
        self.n += 1
        if d > self.top[0]:
            self.top = (d, f"{what} at row {at[0]}, column {at[1]}" if len(at) == 2 else f"{what} at {at}")
        if not d <= tol:
            where = f"row {at[0]}, column {at[1]}" if len(at) == 2 else f"index {at}"
            self.bad.append(f"[{self.prec}] {what}: max |delta| = {d:.3e} > {tol:.1e} at {where}")

    def same_bits(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        self.n += 1
        if got.shape != want.shape or got.dtype != want.dtype:
            self.bad.append(f"[{self.prec}] {what}: {got.dtype}{got.shape} instead of {want.dtype}{want.shape}")
        elif not np.array_equal(got, want):
            diff = np.argwhere(got != want)
            d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
            self.bad.append(f"[{self.prec}] {what}: {len(diff)} of {got.size} values differ in their bits, first at {tuple(int(v) for v in diff[0])}, "
                            f"max |delta| = {d:.3e}")

    def done(self):
        print(f"prims-edges {self.group} [{self.prec}]: {self.n} cases, largest error {self.top[0]:.3e} ({self.top[1]}), {len(self.bad)} missed")
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the line-length cross
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("op", ["shift", "zoom"])
def test_line_length_cross(prec, op, axis):
    """One axis through every length of prims_edge_cases.LENGTHS, the other at 9 (line kernels) and at 70 (float32: the tile kernel as soon
    as the varied side reaches 64 -- 40 for a shift, whose lines are 24 longer)"""
    t = Tally(f"cross {op} axis {axis}", prec)
    fn = S.ndi_shift if op == "shift" else S.ndi_zoom
    for shape in C.cross_shapes(axis):
        for kind in C.KINDS[prec]:
            x = C.image(shape, kind)
            for arg in (C.CROSS_SHIFTS if op == "shift" else C.CROSS_ZOOMS):
                t.close(f"{op} {arg} on {shape[0]} x {shape[1]} ({kind})", fn(x, arg), C.ref(op, shape, arg, kind))
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. batch-driven regimes (the heuristic of prefilter2d: prims_edge_cases, section 2)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", C.BATCHES)
@pytest.mark.parametrize("case", sorted(C.BATCH_CASES))
def test_batch_regimes(prec, case, B):
    """chunk = 64 / 128 / 256 and seg = 2 / 4 / 8 on lines of several chunks / tiles: items 0..15, the last 16 and every 64th against the
    oracle one by one, and four items bit for bit against single-item calls (which run at chunk = 32, seg = 1)"""
    op, arg, (h, w), regime = C.BATCH_CASES[case]
    Hc, Wc = (h + 24, w + 24) if op == "shift" else (h, w)
    t = Tally(f"batch {case} B={B} ({regime} = {C.prefilter_regime(B, Hc, Wc)[0 if regime == 'chunk' else 1]})", prec)
    fn = (lambda v: S.shift_batched(v, arg)) if op == "shift" else (lambda v: S.zoom_batched(v, arg))
    items = C.batch_items(B)
    for kind in C.KINDS[prec]:
        x = C.batch_input(case, kind)[:B]
        xd = torch.from_numpy(x).cuda().to(TORCH_DT[prec])
        out = fn(xd)
        assert tuple(out.shape) == (B, h, w) and out.dtype == TORCH_DT[prec]
        got = out[items].to(torch.float64).cpu().numpy()
        for k, i in enumerate(items):
            t.close(f"{op} {arg} on [{B}, {h}, {w}] item {i} ({kind})", got[k], C.batch_ref(case, kind, i, x[i]))
        for i in C.batch_singles(B):
            t.same_bits(f"{op} {arg} on [{B}, {h}, {w}] item {i} ({kind}) against the single-item call", out[i].cpu().numpy(),
                        fn(xd[i:i + 1].contiguous())[0].cpu().numpy())
        del xd, out
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. blur edges
# ---------------------------------------------------------------------------------------------------------------------------------
def test_blur_edges(prec):
    """Even and non-square kernels (centre at (k - 1) / 2), 1 x 1, 15 x 15, kernels larger than the image, a width one above a 64-lane block"""
    t = Tally("blur", prec)
    for shape in C.BLUR_IMAGES:
        for kk in C.BLUR_KERNELS:
            for kind in C.KINDS[prec]:
                t.close(f"blur {kk[0]} x {kk[1]} on {shape[0]} x {shape[1]} ({kind})", S.blur(C.image(shape, kind), C.blur_kernel(*kk)),
                        C.ref("blur", shape, kk, kind))
    (B, H, W), kk = C.BLUR_BATCH
    for kind in C.KINDS[prec]:
        x = np.stack([C.image((H, W), kind, salt=10 + b) for b in range(B)])
        xd = torch.from_numpy(x).cuda().to(TORCH_DT[prec])
        out = S.blur_batched(xd, C.blur_kernel(*kk))
        for b in range(B):
            t.same_bits(f"blur {kk[0]} x {kk[1]} on [{B}, {H}, {W}] item {b} ({kind}) against the single-item call", out[b].cpu().numpy(),
                        S.blur_batched(xd[b:b + 1].contiguous(), C.blur_kernel(*kk))[0].cpu().numpy())
            t.close(f"blur {kk[0]} x {kk[1]} on [{B}, {H}, {W}] item {b} ({kind})", out[b].cpu().numpy(), O.blur(x[b], C.blur_kernel(*kk)))
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. shift and zoom extremes; forward_model / back_project around Hp = 64
# ---------------------------------------------------------------------------------------------------------------------------------
def test_shift_and_zoom_extremes(prec):
    """No shift, a shift below every rounding, whole and half pixels, a shift past the image (every tap index clamped); zoom by 1 (cc exactly
    integer) to 4; on 1 x 1, one-pixel-wide, 2 x 2, the float horizon and a shape above and on the tile edge"""
    t = Tally("extremes", prec)
    for shape in C.EXTREME_IMAGES:
        for kind in C.KINDS[prec]:
            x = C.image(shape, kind)
            for s in C.extreme_shifts(*shape):
                t.close(f"shift {s} on {shape[0]} x {shape[1]} ({kind})", S.ndi_shift(x, s), C.ref("shift", shape, s, kind))
            for f in C.EXTREME_ZOOMS:
                t.close(f"zoom {f} on {shape[0]} x {shape[1]} ({kind})", S.ndi_zoom(x, f), C.ref("zoom", shape, f, kind))
    t.done()


def test_forward_and_back_projection_edges(prec):
    """H = 39, 40, 41 (H + 24 crosses 64; no multiples of f), W = 67, f = 2 and 3, a fractional and a whole-pixel shift, the asymmetric PSF;
    back_project with an err one row short (padded) and one row long (cropped) of ceil(H / f)"""
    t = Tally("forward / back", prec)
    k = C.fb_psf()
    for H, W, f, s in C.fb_cases():
        for kind in C.KINDS[prec]:
            t.close(f"forward_model f={f} shift {s} on {H} x {W} ({kind})", S.forward_model(C.image((H, W), kind), k, s, f),
                    C.ref("forward", (H, W), (f, s), kind))
            for rows in C.FB_ERR_ROWS:
                err = C.back_err((H, W), (f, s, rows), kind)
                t.close(f"back_project f={f} shift {s} err {err.shape[0]} x {err.shape[1]} -> {H} x {W} ({kind})",
                        S.back_project(err, k, s, f, (H, W)), C.ref("back", (H, W), (f, s, rows), kind))
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. pointwise glue
# ---------------------------------------------------------------------------------------------------------------------------------
def test_mean_frames_bits(prec):
    """mean_frames / mean_frames_batched in the working precision: a sequential sum over r = 0..R-1 divided by R, bit for bit (what
    np.mean(axis=0) of an [R, n] stack does for n > 1; for n = 1 numpy sums pairwise, so the reference is the explicit loop); one sample, and
    one below, on and above a 256-thread block, on fractional data"""
    t = Tally("mean_frames", prec)
    dt = NP_DT[prec]
    rng = np.random.default_rng([C.SEED, 5])
    for R in (1, 7, 40):
        for n in (1, 255, 256, 257):
            st = rng.uniform(0, 255, (3, R, n)).astype(dt)
            want = np.zeros((3, n), dtype=dt)
            for r in range(R):
                want = want + st[:, r]
            want = want / dt(R)
            assert want.dtype == dt
            t.same_bits(f"mean_frames R={R} n={n}", S.mean_frames(st[0].astype(np.float64)).astype(dt), want[0])
            t.same_bits(f"mean_frames_batched B=3 R={R} n={n}", S.mean_frames_batched(st.astype(np.float64)).astype(dt), want)
    t.done()


def test_quantize_u8_edges(prec):
    """+-inf, -0.0 and the neighbours of the bounds in the working precision (no NaN: numpy's own answer is platform-defined)"""
    dt = NP_DT[prec]
    y = np.array([np.inf, -np.inf, -0.0, np.nextafter(dt(256), dt(0)), np.nextafter(dt(255), dt(256)), np.nextafter(dt(0), dt(-1)),
                  np.nextafter(dt(1), dt(0)), np.nextafter(dt(255), dt(0))], dtype=dt)
    got = S.quantize_u8(y.astype(np.float64))
    assert got.dtype == np.uint8 and got.tolist() == [255, 0, 0, 255, 255, 0, 0, 254]
    assert np.array_equal(got, np.clip(y, 0, 255).astype(np.uint8))  # (the clip makes the infinities finite before the cast)


def test_decimate_and_zero_insert_edges(prec):
    """decimate at the last row and column, with a stride larger than the image and on a width one above a 64-lane block; zero_insert onto a
    1 x 1 target"""
    x = C.image((37, 50))
    H, W = x.shape
    for f, py, px in ((2, H - 1, W - 1), (1, H - 1, W - 1), (3, H - 1, 0), (2, 0, W - 1), (100, 0, 0), (100, 36, 49), (51, 1, 1)):
        assert np.array_equal(S.decimate(x, f, py, px), x[py::f, px::f]), (f, py, px)
    x = C.image((5, 65))
    for f, py, px in ((1, 0, 0), (2, 0, 1), (2, 1, 0), (1, 4, 64), (64, 0, 0), (65, 0, 0)):
        assert np.array_equal(S.decimate(x, f, py, px), x[py::f, px::f]), (f, py, px)
    e = C.image((3, 4), salt=2) + 1.0  # no zeros: a dropped sample shows
    for f in (1, 2, 5):
        assert np.array_equal(S.zero_insert(e, f, (1, 1)), e[:1, :1]), f
        assert np.array_equal(S.zero_insert(e[:1, :1], f, (1, 1)), e[:1, :1]), f
    up = np.zeros((2, 66))
    up[0, 0] = e[0, 0]
    assert np.array_equal(S.zero_insert(e[:1, :1], 2, (2, 66)), up)
