"""Pins the integer references of tests/metrics_edge_cases.py to the project's host forms (sr_mi355x.metrics, synth.psnr) at every case
tests/test_gpu_metrics_edges.py holds the kernels of csrc/srx_metrics.hpp to, so that those references are not a second opinion nobody
checked; and asserts the conditions the case tables rely on (every integer sum below 2^53, 0.1 * 250 == 25.0, 128 bins for the bound
case, the live outputs of the local-contrast cases).  A test runs all its cases and reports the failures together.  No GPU."""
import fractions
import warnings

import numpy as np
import pytest

import metrics_edge_cases as C
from sr_mi355x import metrics as M
from sr_mi355x import synth


class Tally:
    def __init__(self):
        self.bad, self.n, self.peak = [], 0, 0

    def check(self, ok, what):
        self.n += 1
        if not ok:
            self.bad.append(what)

    def exact(self, peak, what):
        self.peak = max(self.peak, peak)
        self.check(peak < C.EXACT_BELOW, f"{what}: an integer sum of {peak} is not below 2^53")

    def done(self):
        print(f"{self.n} checks, largest integer sum 2^{np.log2(max(self.peak, 1)):.1f}, {len(self.bad)} missed")
        assert not self.bad, "\n".join(self.bad)


def test_pair_moments_reference_against_psnr_and_psnr_affine():
    """sum (r - t)^2 / n is synth.psnr's mean square to the bit (every square and every partial sum is exact, in numpy's pairwise order as
    in any other); the affine-fit PSNR that follows from the other moments -- formed here in exact rationals -- is metrics.psnr_affine's to
    1e-9 dB wherever the fit is determined (three pixels or more, a test crop that is not constant)"""
    t = Tally()
    for case in C.PAIR_CASES:
        H, W, border, B = case
        for kind in C.KINDS:
            c = C.pair_case(case, kind)
            t.exact(c.peak, f"pair {case} ({kind})")
            for b in range(B):
                crop = (slice(border, H - border), slice(border, W - border))
                r, x = c.ref[b][crop], c.test[b][crop]
                n, st, sr, stt, str_, srr, sdd = c.moments[b]
                t.check(n == r.size and st == x.sum() and sr == r.sum(), f"pair {case} ({kind}) item {b}: n, sum t, sum r")
                want = synth.psnr(r, x)
                got = float("inf") if sdd == 0 else 10.0 * np.log10(255.0 * 255.0 / (sdd / n))
                t.check(got == want, f"pair {case} ({kind}) item {b}: PSNR {got!r} from the moments, synth.psnr {want!r}")
                N, St, Sr, Stt, Str, Srr, _ = (int(v) for v in c.raw[b])
                St, Sr = St // c.scale, Sr // c.scale   # sums of the scaled samples and of their products: the fit's ratios are the samples' own
                den = N * Stt - St * St
                if N < 3 or den == 0:
                    continue
                a = fractions.Fraction(N * Str - St * Sr, den)
                res = fractions.Fraction(N * Srr - Sr * Sr, N) - a * fractions.Fraction(N * Str - St * Sr, N)   # sum (r - a t - b)^2, times scale^2
                mse = float(res / (N * c.scale2)) / 255.0 ** 2
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    want = M.psnr_affine(c.ref[b], c.test[b], border=border)
                got = np.inf if mse == 0 else 10.0 * np.log10(1.0 / mse)
                t.check(abs(got - want) <= 1e-9, f"pair {case} ({kind}) item {b}: affine PSNR {got!r} from the moments, metrics.psnr_affine {want!r}")
    t.done()


def test_local_contrast_reference_against_metrics():
    torch = pytest.importorskip("torch")
    t = Tally()
    assert set(C.LC_LIVE) == set(C.LC_CASES)
    for n, window in C.LC_CASES:
        hw = window // 2
        live = n - 2 * hw if hw > 0 and n >= 2 * hw + 1 else 0
        t.check(live == C.LC_LIVE[(n, window)], f"n {n}, window {window}: {live} outputs inside [hw, n - hw), the table says {C.LC_LIVE[(n, window)]}")
        for kind in C.LC_KINDS:
            x = C.lc_profiles(n, kind)
            got = C.local_contrast_ref(torch.from_numpy(x.copy()), window).numpy()
            for b in range(C.LC_B):
                want = M.local_contrast(x[b], window=window)
                t.check(np.array_equal(got[b], want), f"n {n}, window {window} ({kind}) row {b}: the tensor expression differs from metrics.local_contrast")
                t.check(not got[b][:hw].any() and not got[b][n - hw:].any() and (live > 0 or not got[b].any()),
                        f"n {n}, window {window} ({kind}) row {b}: a non-zero outside [hw, n - hw)")
            if kind == "signed" and live > 100:
                t.check((got < 0).any(), f"n {n}, window {window}: no negative max + min among the signed profiles")
    t.done()


def test_ring_reference_against_radial_average():
    t = Tally()
    for case in C.RING_CASES:
        H, W, cy, cx, nbin = case
        for kind in C.KINDS:
            c = C.ring_case(case, kind)
            t.exact(c.peak, f"ring {case} ({kind})")
            radii, means = M.radial_average(c.img, (cy, cx), nbin)
            want = np.divide(c.sums, c.counts, out=np.zeros(nbin), where=c.counts > 0)
            t.check(len(radii) == nbin and np.array_equal(means, want), f"ring {case} ({kind}): integer sums / counts differ from metrics.radial_average")
        # the integer ring index is the truncated float64 distance, by sqrt as the kernel forms it and by hypot as the host does
        dy, dx = np.arange(H)[:, None] - cy, np.arange(W)[None, :] - cx
        ring = C.ring_index(H, W, cy, cx)
        t.check(np.array_equal(ring, np.sqrt(dx * dx + dy * dy).astype(np.int64)) and np.array_equal(ring, np.hypot(dx, dy).astype(np.int64)),
                f"ring {case}: isqrt differs from the truncated sqrt / hypot")
    on_boundary = C.ring_index(41, 41, 20, 20)
    for dy, dx, k in ((3, 4, 5), (6, 8, 10), (5, 12, 13), (8, 15, 17), (9, 12, 15)):
        t.check(on_boundary[20 + dy, 20 + dx] == k and on_boundary[20 - dx, 20 + dy] == k, f"({dy}, {dx}) is not on ring {k}")
    t.done()


def test_spot_reference_against_subpixel_centre():
    assert 0.1 * C.SPOT_MAX == 25.0 and C.SPOT_EDGE == (24, 25, 26)
    t = Tally()
    for shape in C.SPOT_SHAPES:
        for variant in C.SPOT_VARIANTS:
            c = C.spot_case(shape, variant)
            what = f"spot {shape} ({variant})"
            t.exact(c.peak, what)
            mx, mass, sy, sx = c.out
            t.check(mx == c.img.max(), f"{what}: max")
            if variant.startswith("max_"):
                f, m = c.img.ravel(), c.mask.ravel()
                t.check(mx == C.SPOT_MAX and int((f == mx).sum()) == (2 if variant == "max_both" and f.size > 1 else 1), f"{what}: the planted maximum")
                t.check((variant == "max_last" or f[0] == mx) and (variant == "max_first" or f[-1] == mx), f"{what}: where the maximum sits")
                if f.size >= 5:
                    mid = slice(f.size // 2 - 1, f.size // 2 + 2)
                    t.check(tuple(f[mid]) == C.SPOT_EDGE and tuple(m[mid]) == (False, False, True), f"{what}: 24 and 25 are out, 26 is in")
            if variant in ("zeros", "minus_tens"):
                t.check(not c.mask.any() and mass == 0 and sy == 0 and sx == 0, f"{what}: an empty mask")
                continue
            t.check(c.mask.all() if variant == "nines" else c.mask.any(), f"{what}: the mask")
            t.check((float(sy / mass), float(sx / mass)) == M.subpixel_centre(c.img), f"{what}: sum p y / sum p, sum p x / sum p differ from metrics.subpixel_centre")
    t.done()


def test_magnitude_cases():
    """(the reference IS metrics._gaussian_filter / _sobel: what remains to pin is what the table says about the cases)"""
    radius = {s: int(4.0 * s + 0.5) for s, _ in C.MAG_CASES}
    assert radius == {1.5: 6, 0.5: 2, 2.0: 8, 2.1: 8} and int(4.0 * C.MAG_REFUSED_SIGMA + 0.5) == 9
    assert not C.mag_case(1.5, (1, 1)).mag.any()
    assert 8 > 5   # (5, 33) at radius 8: one fold reaches rows -1 .. -5, rows -6 .. -8 fold again at the far end
    for sigma, shape in C.MAG_CASES:
        c = C.mag_case(sigma, shape)
        assert c.mag.shape == shape and np.isfinite(c.mag).all() and (shape == (1, 1) or c.mag.any())


def slanted_edge_bins(roi, dist, bw):
    """the binning block of metrics.slanted_edge_esf, with its bin width a parameter -> per-bin counts and means (nan: empty)"""
    fd, fv = dist.ravel(), roi.ravel().astype(np.float64)
    keep = (fd > -8) & (fd < 10)
    fd, fv = fd[keep], fv[keep]
    bins = np.arange(fd.min(), fd.max() + bw, bw)
    esf_x = 0.5 * (bins[:-1] + bins[1:])
    which = np.searchsorted(bins, fd, side="right") - 1
    ok = (which >= 0) & (which < len(esf_x))
    cnt = np.bincount(which[ok], minlength=len(esf_x)).astype(np.float64)
    esf_y = np.full(len(esf_x), np.nan)
    for i in np.nonzero(cnt)[0]:
        esf_y[i] = fv[ok][which[ok] == i].mean()
    return cnt, esf_y


def test_bins_reference_against_slanted_edge_esf():
    t = Tally()
    empty = [c for c in C.EDGE_CASES if C.edge_range(c)[1] is None]
    assert empty == [(1, 300, 0.02, 150.0, 0, 0.25), (24, 40, 0.0, 1000.0, 1, None)]
    assert C.edge_case(C.BINS_BOUND_CASE, "int").nbin == C.EDGE_MAX_BINS == 128
    assert C.edge_case((24, 40, 0.0, 12.0, 1, 18.0), "int").nbin == 1
    for case in C.edge_bin_cases():
        H, W, m, b, rows_are_x, bw = case
        dist, norm = C.edge_dist(H, W, m, b, rows_are_x)
        for kind in C.KINDS:
            c = C.edge_case(case, kind)
            what = f"bins {case} ({kind})"
            t.exact(c.peak, what)
            t.check(c.norm == norm and -8 < c.lo <= c.hi < 10 and 1 <= c.nbin <= C.EDGE_MAX_BINS, f"{what}: lo {c.lo}, hi {c.hi}, {c.nbin} bins")
            cnt, mean = slanted_edge_bins(c.roi, dist, bw)
            t.check(len(cnt) == c.nbin and np.array_equal(cnt, c.counts), f"{what}: the counts differ from slanted_edge_esf's")
            full = c.counts > 0
            got = c.sums[full] / c.counts[full]
            t.check(len(cnt) == c.nbin and np.all(np.abs(got - mean[full]) <= 1e-12 * np.abs(mean[full])), f"{what}: sum / count differs from the per-bin mean")
            t.check(c.counts.sum() + c.dropped == c.kept.sum(), f"{what}: pixels lost")
    # the first case: every distance an integer, -8 and 10 out, each kept pixel on the lower edge of its bin, the pixels at hi in no bin
    c = C.edge_case(C.EDGE_CASES[0], "int")
    t.check((c.lo, c.hi, c.nbin) == (-7.0, 9.0, 64) and np.array_equal(c.dist, np.rint(c.dist)) and c.dropped == 24, "the integer-distance case")
    t.check(np.array_equal(c.counts, np.where(np.arange(64) % 4 == 0, 24.0, 0.0)), "the integer-distance case: 24 pixels in every fourth bin")
    t.done()
