"""The metric reductions of csrc/srx_metrics.hpp at the hand-overs of their code: srx_pair_moments_*, srx_local_contrast_*, srx_ring_sums_*,
srx_spot_moments_*, srx_edge_magnitude_f64, srx_edge_dist_range and srx_edge_bins_*, called RAW through the C ABI (the wrappers of
sr_mi355x.metrics_device hide the raw sums and have no float32 form of two of the calls), against the exact references of
tests/metrics_edge_cases.py (pinned to sr_mi355x.metrics on the same cases by tests/test_metrics_edges_host.py).  The cases and what each
is there for: tests/metrics_edge_cases.py.

Every comparison is np.array_equal (the inputs make every sum exact in float64 in any order); the one tolerance is the magnitude's 1e-11 DN.
Every output is poisoned with NaN before its call, so a value the kernel did not store shows.  A test runs all its cases and then fails
with one line per case that missed.  Once per entry point the same call is made twice and must give the same bits; for pair_moments and
local_contrast, item b of a batch must have the bits of a B = 1 call on item b.  Every refusal of the host checks is asserted with its
status and with its poisoned outputs untouched.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from sr_mi355x import _lib, api  # noqa: E402

import metrics_edge_cases as C  # noqa: E402

DT = {"f32": torch.float32, "f64": torch.float64}
PRECS = ("f32", "f64")
POISON = float("nan")


@pytest.fixture(params=PRECS)
def prec(request):
    return request.param


def L():
    return _lib.load()


def dev(a, prec="f64"):
    """host float64 array -> contiguous device tensor of the precision (every sample of the case module is exact in float32)"""
    h = torch.from_numpy(np.array(a, dtype=np.float64))   # (a copy: the case module hands its arrays out read-only)
    t = h.cuda().to(DT[prec]).contiguous()
    assert torch.equal(t.to(torch.float64).cpu(), h)
    return t


def poisoned(shape, dtype=torch.float64):
    return torch.full(shape, POISON, dtype=dtype, device="cuda")


def host(t):
    torch.cuda.synchronize()
    return t.to(torch.float64).cpu().numpy() if t.dtype != torch.float64 else t.cpu().numpy()


def ws(B, H, W, nbin):
    """an arena of srx_metrics_workspace_bytes at the call's own arguments"""
    return api._ws(L().srx_metrics_workspace_bytes(B, H, W, nbin))


class Tally:
    """Collects the cases of one test: a line per case that missed"""

    def __init__(self, group, prec="f64"):
        self.group, self.prec, self.bad, self.n, self.top = group, prec, [], 0, 0.0

    def status(self, what, st, want=_lib.OK):
        self.n += 1
        if st != want:
            self.bad.append(f"[{self.prec}] {what}: status {st} instead of {want}")
        return st == want

    def same(self, what, got, want):
        got, want = np.asarray(got), np.asarray(want)
        self.n += 1
        if got.shape != want.shape or got.dtype != want.dtype:
            self.bad.append(f"[{self.prec}] {what}: {got.dtype}{got.shape} instead of {want.dtype}{want.shape}")
        elif not np.array_equal(got, want):
            diff = np.argwhere(~(got == want))
            at = tuple(int(v) for v in diff[0])
            self.bad.append(f"[{self.prec}] {what}: {len(diff)} of {got.size} values differ, first at {at}: {got[at]!r} instead of {want[at]!r}")

    def close(self, what, got, want, tol):
        self.n += 1
        d = np.abs(np.asarray(got) - np.asarray(want))
        top = float(d.max()) if np.isfinite(d).all() else float("inf")
        self.top = max(self.top, top)
        if got.shape != want.shape or not top <= tol:
            self.bad.append(f"[{self.prec}] {what}: max |delta| = {top:.3e} > {tol:.1e} at {np.unravel_index(int(np.nanargmax(d)), d.shape)}")

    def done(self):
        print(f"metrics-edges {self.group} [{self.prec}]: {self.n} checks, largest error {self.top:.3e}, {len(self.bad)} missed")
        assert not self.bad, "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the raw calls: -> (status, host float64 array of the poisoned output)
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_moments(prec, ref, test, border):
    B, H, W = ref.shape
    r, t, out = dev(ref, prec), dev(test, prec), poisoned((B, 7))
    w, wp, wn = ws(B, H, W, 1)
    st = api._fn("srx_pair_moments", prec)(api._p(r), api._p(t), B, H, W, border, api._p(out), wp, wn, api._stream())
    return st, host(out)


def local_contrast(prec, prof, window):
    B, n = prof.shape
    x, out = dev(prof, prec), poisoned((B, n), DT[prec])
    st = api._fn("srx_local_contrast", prec)(api._p(x), B, n, window, api._p(out), api._stream())
    torch.cuda.synchronize()
    return st, out.cpu()


def ring_sums(prec, img, cy, cx, nbin):
    H, W = img.shape
    x, out = dev(img, prec), poisoned((2 * nbin,))
    w, wp, wn = ws(1, H, W, nbin)
    st = api._fn("srx_ring_sums", prec)(api._p(x), H, W, float(cy), float(cx), nbin, api._p(out), wp, wn, api._stream())
    return st, host(out)


def spot_moments(prec, img):
    H, W = img.shape
    x, out = dev(img, prec), poisoned((4,))
    st = api._fn("srx_spot_moments", prec)(api._p(x), H, W, api._p(out), api._stream())
    return st, host(out)


def edge_magnitude(roi, sigma):
    H, W = roi.shape
    x, out = dev(roi), poisoned((H, W))
    w, wp, wn = ws(1, H, W, 1)
    st = L().srx_edge_magnitude_f64(api._p(x), H, W, sigma, api._p(out), wp, wn, api._stream())
    return st, host(out)


def edge_dist_range(H, W, m, b, norm, rows_are_x):
    out = poisoned((2,))
    st = L().srx_edge_dist_range(H, W, m, b, norm, rows_are_x, api._p(out), api._stream())
    return st, host(out)


def edge_bins(prec, roi, m, b, norm, rows_are_x, lo, bw, nbin):
    H, W = roi.shape
    x, out = dev(roi, prec), poisoned((2 * max(nbin, 1),))
    w, wp, wn = ws(1, H, W, nbin)
    st = api._fn("srx_edge_bins", prec)(api._p(x), H, W, m, b, norm, rows_are_x, lo, bw, nbin, api._p(out), wp, wn, api._stream())
    return st, host(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. pair_moments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pair_moments(prec):
    t = Tally("pair_moments", prec)
    for case in C.PAIR_CASES:
        for kind in C.KINDS:
            c = C.pair_case(case, kind)
            st, got = pair_moments(prec, c.ref, c.test, case[2])
            if t.status(f"pair_moments {case} ({kind})", st):
                t.same(f"pair_moments {case} ({kind})", got, c.moments)
    H, W, border, B = C.PAIR_REFUSED_CASE   # (the table's row whose border leaves no column)
    c = C.pair_case((H, 7, border, B), "int")
    st, got = pair_moments(prec, c.ref[:, :, :W], c.test[:, :, :W], border)
    t.status(f"pair_moments {C.PAIR_REFUSED_CASE}: 2 border >= W", st, _lib.E_INVALID)
    t.same(f"pair_moments {C.PAIR_REFUSED_CASE}: a refused call stored", np.isnan(got), np.ones((B, 7), dtype=bool))
    # the same call twice; item b of a batch against a B = 1 call on item b
    for kind in C.KINDS:
        c = C.pair_case(C.PAIR_BATCH_CASE, kind)
        border = C.PAIR_BATCH_CASE[2]
        _, first = pair_moments(prec, c.ref, c.test, border)
        t.same(f"pair_moments {C.PAIR_BATCH_CASE} ({kind}) a second time", pair_moments(prec, c.ref, c.test, border)[1], first)
        for b in range(C.PAIR_BATCH_CASE[3]):
            t.same(f"pair_moments {C.PAIR_BATCH_CASE} ({kind}) item {b} against the single-item call",
                   pair_moments(prec, c.ref[b:b + 1], c.test[b:b + 1], border)[1][0], first[b])
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. local_contrast
# ---------------------------------------------------------------------------------------------------------------------------------
def test_local_contrast(prec):
    t = Tally("local_contrast", prec)
    for n, window in C.LC_CASES:
        for kind in C.LC_KINDS:
            x = C.lc_profiles(n, kind)
            want = C.local_contrast_ref(torch.from_numpy(x.copy()).to(DT[prec]), window)   # on the CPU, in the kernel's precision
            st, got = local_contrast(prec, x, window)
            if t.status(f"local_contrast n {n} window {window} ({kind})", st):
                t.same(f"local_contrast n {n} window {window} ({kind})", got.numpy(), want.numpy())
    for kind in ("frac", "signed"):
        x = C.lc_profiles(257, kind)
        _, first = local_contrast(prec, x, 16)
        t.same(f"local_contrast n 257 window 16 ({kind}) a second time", local_contrast(prec, x, 16)[1].numpy(), first.numpy())
        for b in range(C.LC_B):
            t.same(f"local_contrast n 257 window 16 ({kind}) row {b} against the single-row call", local_contrast(prec, x[b:b + 1], 16)[1][0].numpy(),
                   first[b].numpy())
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ring_sums: the raw sums and counts
# ---------------------------------------------------------------------------------------------------------------------------------
def test_ring_sums(prec):
    t = Tally("ring_sums", prec)
    for case in C.RING_CASES:
        H, W, cy, cx, nbin = case
        for kind in C.KINDS:
            c = C.ring_case(case, kind)
            st, got = ring_sums(prec, c.img, cy, cx, nbin)
            if t.status(f"ring_sums {case} ({kind})", st):
                t.same(f"ring_sums {case} ({kind}) sums", got[:nbin], c.sums)
                t.same(f"ring_sums {case} ({kind}) counts", got[nbin:], c.counts)
    H, W, cy, cx, nbin = case = C.RING_CASES[2]
    c = C.ring_case(case, "frac")
    t.same(f"ring_sums {case} a second time", ring_sums(prec, c.img, cy, cx, nbin)[1], ring_sums(prec, c.img, cy, cx, nbin)[1])
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. spot_moments: the four raw outputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_spot_moments(prec):
    t = Tally("spot_moments", prec)
    for shape in C.SPOT_SHAPES:
        for variant in C.SPOT_VARIANTS:
            c = C.spot_case(shape, variant)
            st, got = spot_moments(prec, c.img)
            if t.status(f"spot_moments {shape} ({variant})", st):
                t.same(f"spot_moments {shape} ({variant}) {{max, sum p, sum p y, sum p x}}", got, c.out)
    c = C.spot_case((300, 7), "frac")
    t.same("spot_moments (300, 7) (frac) a second time", spot_moments(prec, c.img)[1], spot_moments(prec, c.img)[1])
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. edge_magnitude (float64 only)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_edge_magnitude():
    t = Tally("edge_magnitude")
    for sigma, shape in C.MAG_CASES:
        c = C.mag_case(sigma, shape)
        st, got = edge_magnitude(c.roi, sigma)
        if t.status(f"edge_magnitude sigma {sigma} on {shape}", st):
            t.close(f"edge_magnitude sigma {sigma} on {shape}", got, c.mag, C.MAG_TOL)
    st, got = edge_magnitude(C.mag_case(1.5, (1, 1)).roi, 1.5)
    t.same("edge_magnitude of one pixel", got, np.zeros((1, 1)))
    c = C.mag_case(2.0, (5, 33))
    t.same("edge_magnitude sigma 2.0 on (5, 33) a second time", edge_magnitude(c.roi, 2.0)[1], edge_magnitude(c.roi, 2.0)[1])
    st, got = edge_magnitude(c.roi, C.MAG_REFUSED_SIGMA)
    t.status(f"edge_magnitude sigma {C.MAG_REFUSED_SIGMA}", st, _lib.E_UNSUPPORTED)
    t.same(f"edge_magnitude sigma {C.MAG_REFUSED_SIGMA}: a refused call stored", np.isnan(got), np.ones((5, 33), dtype=bool))
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. edge_dist_range / edge_bins
# ---------------------------------------------------------------------------------------------------------------------------------
def test_edge_dist_range():
    t = Tally("edge_dist_range")
    for case in C.EDGE_CASES:
        H, W, m, b, rows_are_x, _ = case
        norm, rng = C.edge_range(case)
        st, got = edge_dist_range(H, W, m, b, norm, rows_are_x)
        if t.status(f"edge_dist_range {case}", st):
            t.same(f"edge_dist_range {case}", got, np.array(C.EDGE_EMPTY_RANGE if rng is None else rng))
    H, W, m, b, rows_are_x, _ = case = C.EDGE_CASES[2]
    norm = C.edge_range(case)[0]
    t.same(f"edge_dist_range {case} a second time", edge_dist_range(H, W, m, b, norm, rows_are_x)[1], edge_dist_range(H, W, m, b, norm, rows_are_x)[1])
    t.done()


def test_edge_bins(prec):
    t = Tally("edge_bins", prec)
    for case in C.edge_bin_cases():
        H, W, m, b, rows_are_x, bw = case
        for kind in C.KINDS:
            c = C.edge_case(case, kind)
            st, got = edge_bins(prec, c.roi, m, b, c.norm, rows_are_x, c.lo, bw, c.nbin)
            if t.status(f"edge_bins {case} ({kind})", st):
                t.same(f"edge_bins {case} ({kind}) sums", got[:c.nbin], c.sums)
                t.same(f"edge_bins {case} ({kind}) counts", got[c.nbin:], c.counts)
    # the bound: 128 bins pass (above), 129 on the same data are refused
    H, W, m, b, rows_are_x, bw = C.BINS_BOUND_CASE
    c = C.edge_case(C.BINS_BOUND_CASE, "frac")
    assert c.nbin == C.EDGE_MAX_BINS
    t.same(f"edge_bins {C.BINS_BOUND_CASE} a second time", edge_bins(prec, c.roi, m, b, c.norm, rows_are_x, c.lo, bw, c.nbin)[1],
           edge_bins(prec, c.roi, m, b, c.norm, rows_are_x, c.lo, bw, c.nbin)[1])
    st, got = edge_bins(prec, c.roi, m, b, c.norm, rows_are_x, c.lo, bw, c.nbin + 1)
    t.status(f"edge_bins {C.BINS_BOUND_CASE} with 129 bins", st, _lib.E_INVALID)
    t.same("edge_bins with 129 bins: a refused call stored", np.isnan(got), np.ones(2 * 129, dtype=bool))
    t.done()


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. refusals: decided on the host before anything is queued -- the status, and the poisoned outputs untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(prec):
    t = Tally("refusals", prec)
    st_ = api._stream()
    x = dev(C.values(C.ints((9, 9), "int", 8), "int"), prec)
    out = poisoned((2 * 4097,))
    w, wp, wn = api._ws(1 << 20)
    p, fn = api._p, lambda name: api._fn(name, prec)  # noqa: E731
    e = _lib.E_INVALID
    calls = [
        ("pair_moments 2 border >= H", e, lambda: fn("srx_pair_moments")(p(x), p(x), 1, 4, 9, 2, p(out), wp, wn, st_)),
        ("pair_moments 2 border >= W", e, lambda: fn("srx_pair_moments")(p(x), p(x), 1, 9, 4, 2, p(out), wp, wn, st_)),
        ("pair_moments border < 0", e, lambda: fn("srx_pair_moments")(p(x), p(x), 1, 9, 9, -1, p(out), wp, wn, st_)),
        ("pair_moments B = 65536", _lib.E_UNSUPPORTED, lambda: fn("srx_pair_moments")(p(x), p(x), 65536, 1, 1, 0, p(out), wp, wn, st_)),
        ("local_contrast window < 0", e, lambda: fn("srx_local_contrast")(p(x), 1, 81, -1, p(out), st_)),
        ("local_contrast B = 65536", _lib.E_UNSUPPORTED, lambda: fn("srx_local_contrast")(p(x), 65536, 1, 2, p(out), st_)),
        ("ring_sums nbin = 0", e, lambda: fn("srx_ring_sums")(p(x), 9, 9, 4.0, 4.0, 0, p(out), wp, wn, st_)),
        ("ring_sums nbin = 4097", e, lambda: fn("srx_ring_sums")(p(x), 9, 9, 4.0, 4.0, 4097, p(out), wp, wn, st_)),
        ("spot_moments 4097 x 4096", e, lambda: fn("srx_spot_moments")(p(x), 4097, 4096, p(out), st_)),
        ("edge_bins nbin = 0", e, lambda: fn("srx_edge_bins")(p(x), 9, 9, 0.0, 4.0, 1.0, 1, -4.0, 0.25, 0, p(out), wp, wn, st_)),
        ("edge_bins nbin = 129", e, lambda: fn("srx_edge_bins")(p(x), 9, 9, 0.0, 4.0, 1.0, 1, -4.0, 0.25, 129, p(out), wp, wn, st_)),
        ("edge_bins norm = 0", e, lambda: fn("srx_edge_bins")(p(x), 9, 9, 0.0, 4.0, 0.0, 1, -4.0, 0.25, 16, p(out), wp, wn, st_)),
        ("edge_bins bw = 0", e, lambda: fn("srx_edge_bins")(p(x), 9, 9, 0.0, 4.0, 1.0, 1, -4.0, 0.0, 16, p(out), wp, wn, st_)),
    ]
    if prec == "f64":   # the entry points without a float32 form
        xd = x
        calls += [
            ("edge_magnitude sigma = 0", e, lambda: L().srx_edge_magnitude_f64(p(xd), 9, 9, 0.0, p(out), wp, wn, st_)),
            ("edge_magnitude sigma = 2.2", _lib.E_UNSUPPORTED, lambda: L().srx_edge_magnitude_f64(p(xd), 9, 9, C.MAG_REFUSED_SIGMA, p(out), wp, wn, st_)),
            ("edge_dist_range norm = 0", e, lambda: L().srx_edge_dist_range(9, 9, 0.0, 4.0, 0.0, 1, p(out), st_)),
            ("edge_dist_range 4097 x 4096", e, lambda: L().srx_edge_dist_range(4097, 4096, 0.0, 4.0, 1.0, 1, p(out), st_)),
        ]
    for what, want, call in calls:
        st = call()
        torch.cuda.synchronize()
        t.status(what, st, want)
        t.n += 1
        if not bool(torch.isnan(out).all()):
            t.bad.append(f"[{prec}] {what}: a refused call stored into its output")
            out.fill_(POISON)
    t.done()
