"""Case tables, inputs and exact references shared by tests/test_metrics_edges_host.py (no GPU: the references against sr_mi355x.metrics)
and tests/test_gpu_metrics_edges.py (the kernels of csrc/srx_metrics.hpp against the references).  A plain helper module like
prims_edge_cases.py: numpy only, nothing registered.

The cases sit where the kernels hand over:

  k_pair_moments      nblk = min(1024, h) blocks of rows_per = ceil(h / nblk) rows (trailing blocks own no row), columns in strides of 256
                      with a tail, the item stride H W under a border
  k_local_contrast    hw = window / 2 == 0 and n < 2 hw + 1 give zeros, the live range [hw, n - hw) of one output, the 256-thread block edge
  k_ring_rows / k_ring_sum   2 nbin doubles of dynamic LDS zeroed and stored in strides of 256 (nbin up to 4096: 64 KiB), the truncation of a
                      distance that is exactly an integer, centres off the image
  k_spot_moments      y = i / W on non-square images, H W below, at and above 256, the strict p > 0.1 max in float64, ties of the maximum
  k_correlate1d / k_sobel_mag   64 x 4 blocks, reflect_idx folding more than once when a side is shorter than the Gaussian radius
  k_edge_bins_rows    a thread per bin (at most 128), closed-open bins with pixels exactly on an edge, the open interval (-8, 10)
  k_edge_dist_range   its answer when no pixel qualifies

Inputs.  Seeded samples of two kinds: "int" = integers(0, 256) and "frac" = integers(0, 2041) / 8 (local contrast adds "signed" =
integers(-2040, 2041) / 8 and constant profiles).  All are exact in float32, and every sum a kernel forms from them is a dyadic rational far
below 2^53 (every reference reports the largest integer it formed as `peak`; the host test asserts the bound): exact in float64 in ANY
order.  So the references are sums of numpy int64 on the samples scaled by 8 (products: by 64), divided once, and every comparison but
the magnitude's is np.array_equal.  Every reference is computed once per process and handed out read-only.
"""
import functools
import math
import types

import numpy as np

from sr_mi355x import metrics as M

SEED = 4597
KINDS = ("int", "frac")
SCALE = {"int": 1, "frac": 8, "signed": 8}
_RANGE = {"int": (0, 256), "frac": (0, 2041), "signed": (-2040, 2041)}
_KIND_ID = {"int": 0, "frac": 1, "signed": 2, "const": 3}
EXACT_BELOW = 2 ** 53


def ints(shape, kind, *salt):
    """the samples of `kind` times SCALE[kind], int64"""
    lo, hi = _RANGE[kind]
    return np.random.default_rng([SEED, _KIND_ID[kind], *salt]).integers(lo, hi, shape, dtype=np.int64)


def values(q, kind):
    """... and the samples themselves, float64 (exact in float32 as well)"""
    return q.astype(np.float64) / float(SCALE[kind])


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _case(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. pair_moments: (H, W, border, B)
# ---------------------------------------------------------------------------------------------------------------------------------
PAIR_CASES = (
    (1, 1, 0, 1),        # smallest image
    (3, 3, 1, 1),        # crop of one pixel
    (2, 2, 0, 2),        # smallest batch
    (5, 255, 0, 1), (5, 256, 0, 1), (5, 257, 0, 1),   # around the 256-column stride
    (4, 523, 0, 1),      # two strides and a tail
    (9, 300, 4, 1),      # one interior row under a border
    (1024, 3, 0, 1),     # nblk = 1024 with one row each
    (1025, 3, 0, 1),     # rows_per = 2: 513 working blocks and 511 empty ones
    (1030, 7, 3, 2),     # h = 1024 under a border, in a batch (one interior column)
    (2049, 2, 0, 1),     # rows_per = 3
    (61, 97, 3, 3),      # three different items
)
# h = 1024 under a border as first written down: five columns leave none inside a border of 3 (2 border >= W), so the call is refused with
# SRX_E_INVALID and this row is asserted as that refusal; (1030, 7, 3, 2) above is the nearest shape that reaches the kernel
PAIR_REFUSED_CASE = (1030, 5, 3, 2)
PAIR_BATCH_CASE = (61, 97, 3, 3)   # item b of this batch against a B = 1 call on item b


@functools.lru_cache(maxsize=None)
def pair_case(case, kind):
    """-> ref, test float64 [B, H, W]; moments float64 [B, 7] = {n, sum t, sum r, sum t^2, sum t r, sum r^2, sum (r - t)^2} over rows /
    columns [border, size - border), from int64 sums; peak"""
    H, W, border, B = case
    q = ints((2, B, H, W), kind, 1, H, W, border, B)
    r, t = (q[i][:, border:H - border, border:W - border] for i in (0, 1))
    assert r.shape == (B, H - 2 * border, W - 2 * border)
    s = SCALE[kind]
    ax = (1, 2)
    raw = np.stack([np.full(B, r[0].size, dtype=np.int64), t.sum(ax) * s, r.sum(ax) * s, (t * t).sum(ax), (t * r).sum(ax), (r * r).sum(ax),
                    ((r - t) ** 2).sum(ax)], axis=1)   # all times s^2 (the count apart)
    mom = raw.astype(np.float64) / float(s * s)
    mom[:, 0] = raw[:, 0]
    return _case(ref=values(q[0], kind), test=values(q[1], kind), moments=mom, raw=raw, scale=s, scale2=s * s, peak=int(np.abs(raw).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. local_contrast: (n, window), B = 3
# ---------------------------------------------------------------------------------------------------------------------------------
LC_CASES = (
    (1, 0), (5, 0), (5, 1),    # hw = 0: zeros
    (2, 2),                    # shorter than 2 hw + 1: zeros
    (3, 2), (21, 20), (21, 21), (601, 600),   # exactly one non-zero output
    (20, 20),                  # zeros
    (256, 16), (257, 16),      # block edge
    (600, 300),                # long window
)
LC_KINDS = ("int", "frac", "signed", "const")
LC_B = 3
LC_CONST = (37.5, 0.0, -4.25)   # (the last: max + min < 0)
# outputs inside [hw, n - hw), the only ones the kernel computes
LC_LIVE = {(1, 0): 0, (5, 0): 0, (5, 1): 0, (2, 2): 0, (3, 2): 1, (21, 20): 1, (21, 21): 1, (601, 600): 1, (20, 20): 0, (256, 16): 240, (257, 16): 241,
           (600, 300): 300}


@functools.lru_cache(maxsize=None)
def lc_profiles(n, kind):
    """float64 [LC_B, n]"""
    if kind == "const":
        return _ro(np.repeat(np.array(LC_CONST)[:, None], n, axis=1))
    return _ro(values(ints((LC_B, n), kind, 2, n), kind))


def local_contrast_ref(x, window):
    """metrics.local_contrast on a torch tensor [B, n], in the tensor's own precision (the expression of
    test_gpu_memory_contract._local_contrast_ref, on tensor methods only: this module does not import torch): (max - min) /
    (max + min + 1e-9) of profile[i - w/2 : i + w/2], 0 within w/2 of either end.  Maxima, one subtraction, two additions and one correctly
    rounded division: the kernel's result bit for bit."""
    B, n = x.shape
    hw, res = window // 2, x.new_zeros(x.shape)
    if hw > 0 and n >= 2 * hw + 1:
        win = x.unfold(1, 2 * hw, 1)[:, :n - 2 * hw]   # window s = profile[s : s + 2 hw] belongs to i = s + hw, i < n - hw
        mx, mn = win.max(dim=2).values, win.min(dim=2).values
        res[:, hw:n - hw] = (mx - mn) / (mx + mn + x.new_tensor(1e-9))
    return res


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. ring_sums: (H, W, cy, cx, nbin), centres on multiples of 1/4 px
# ---------------------------------------------------------------------------------------------------------------------------------
RING_CASES = (
    (41, 41, 20, 20, 20),         # integer centre: the 3-4-5, 6-8-10, 5-12-13, 8-15-17, 9-12-15 pixels sit exactly on a ring boundary
    (41, 41, 20.5, 20.5, 20),     # half-integer centre
    (8, 700, 4, 0, 600),          # nbin > 256: LDS strides and three blocks of k_ring_sum
    (4, 64, 2, 32, 4096),         # the largest nbin, mostly empty rings
    (1, 1, 0, 0, 1),              # smallest image
    (300, 1, 150, 0.5, 150),      # one column
    (61, 97, -3.5, 99, 40),       # centre off the image
    (64, 64, 31.75, 32.25, 5),    # most pixels beyond nbin
    (37, 53, 18.25, 26.75, 18),   # odd shape, quarter-pixel centre
)
_isqrt = np.vectorize(math.isqrt, otypes=[np.int64])


def ring_index(H, W, cy, cx):
    """floor(sqrt((y - cy)^2 + (x - cx)^2)) per pixel in integers: with d2 = (4 y - 4 cy)^2 + (4 x - 4 cx)^2 = 16 d^2,
    floor(d) = isqrt(floor(d^2)) = isqrt(d2 // 16).  (A non-integer distance stays at least 1 / (32 k) away from the integer k, far above
    the rounding of a float64 square root: the kernel's truncation is unambiguous.)"""
    cy4, cx4 = int(4 * cy), int(4 * cx)
    assert cy4 == 4 * cy and cx4 == 4 * cx
    dy, dx = 4 * np.arange(H, dtype=np.int64) - cy4, 4 * np.arange(W, dtype=np.int64) - cx4
    return _isqrt((dy[:, None] ** 2 + dx[None, :] ** 2) // 16)


@functools.lru_cache(maxsize=None)
def ring_case(case, kind):
    """-> img float64 [H, W]; sums, counts float64 [nbin] per ring, from integers; peak"""
    H, W, cy, cx, nbin = case
    q = ints((H, W), kind, 3, H, W, nbin)
    ring = ring_index(H, W, cy, cx).ravel()
    inside = ring < nbin
    tot, cnt = np.zeros(nbin, dtype=np.int64), np.zeros(nbin, dtype=np.int64)
    np.add.at(tot, ring[inside], q.ravel()[inside])
    np.add.at(cnt, ring[inside], 1)
    return _case(img=values(q, kind), sums=tot.astype(np.float64) / float(SCALE[kind]), counts=cnt.astype(np.float64), peak=int(tot.max(initial=0)))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. spot_moments: shapes x variants
# ---------------------------------------------------------------------------------------------------------------------------------
SPOT_SHAPES = ((1, 1), (3, 5), (16, 16), (1, 257), (257, 1), (7, 300), (300, 7), (600, 700))
# a base of integers(0, 250) with the maximum 250 planted at the first sample, at the last, at both (a tie), and 24, 25, 26 planted in the
# middle (0.1 * 250 == 25.0 in float64: 25 is excluded, 26 kept; images of fewer than 5 samples have no room for them);
# constants: 0 (nothing above 0.1 max = 0), 9 (everything), -10 (0.1 max = -1: an empty mask, mass 0, max -10); one "frac" image
SPOT_VARIANTS = ("max_first", "max_last", "max_both", "zeros", "nines", "minus_tens", "frac")
SPOT_MAX, SPOT_EDGE = 250, (24, 25, 26)


@functools.lru_cache(maxsize=None)
def spot_case(shape, variant):
    """-> img float64 [H, W]; out float64 [4] = {max, sum p, sum p y, sum p x over p > 0.1 max}; the mask; peak"""
    H, W = shape
    n, s = H * W, 1
    if variant == "frac":
        q, s = ints((H, W), "frac", 4, H, W), SCALE["frac"]
    elif variant in ("zeros", "nines", "minus_tens"):
        q = np.full((H, W), {"zeros": 0, "nines": 9, "minus_tens": -10}[variant], dtype=np.int64)
    else:
        q = np.random.default_rng([SEED, 5, H, W]).integers(0, SPOT_MAX, (H, W), dtype=np.int64)
        f = q.reshape(-1)
        if n >= 5:
            f[n // 2 - 1:n // 2 + 2] = SPOT_EDGE
        if variant in ("max_first", "max_both"):
            f[0] = SPOT_MAX
        if variant in ("max_last", "max_both"):
            f[n - 1] = SPOT_MAX
    img = q.astype(np.float64) / float(s)
    mx = float(img.max())
    mask = img > 0.1 * mx   # the product in float64, as metrics.subpixel_centre forms it
    yy, xx = np.mgrid[:H, :W]
    raw = [int(q[mask].sum()), int((q * yy)[mask].sum()), int((q * xx)[mask].sum())]
    return _case(img=img, out=np.array([mx] + [v / float(s) for v in raw]), mask=mask, peak=max(abs(v) for v in raw))


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. edge_magnitude: (sigma, (H, W)); radius = int(4 sigma + 0.5)
# ---------------------------------------------------------------------------------------------------------------------------------
MAG_CASES = (
    (1.5, (1, 1)),     # radius 6; one pixel: the result is 0
    (1.5, (1, 40)), (1.5, (40, 1)), (1.5, (2, 37)), (1.5, (3, 3)), (1.5, (5, 64)), (1.5, (6, 65)), (1.5, (7, 63)), (1.5, (13, 13)), (1.5, (4, 257)),
    (0.5, (9, 70)),    # radius 2
    (2.0, (5, 33)),    # radius 8 on 5 rows: the index folds twice
    (2.0, (17, 17)),
    (2.1, (20, 20)),   # the largest sigma accepted (4 sigma + 0.5 < 9)
)
MAG_TOL = 1e-11        # DN on the 0..255 scale: what tests/test_gpu_metrics.py holds srx_edge_magnitude_f64 to
MAG_REFUSED_SIGMA = 2.2   # radius 9: SRX_E_UNSUPPORTED


@functools.lru_cache(maxsize=None)
def mag_case(sigma, shape):
    """-> roi float64 [H, W] ("int"); mag = sqrt(_sobel(., 1)^2 + _sobel(., 0)^2) of metrics._gaussian_filter(roi, sigma)"""
    roi = values(ints(shape, "int", 6, *shape), "int")
    smooth = M._gaussian_filter(roi, sigma)
    return _case(roi=roi, mag=np.sqrt(M._sobel(smooth, 1) ** 2 + M._sobel(smooth, 0) ** 2))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. edge_dist_range / edge_bins: (H, W, m, b, rows_are_x, bw); the line is given, norm = sqrt(1 + m^2)
# ---------------------------------------------------------------------------------------------------------------------------------
BINS_BOUND_CASE = (40, 64, 0.1, 28.8, 1, 0.140625)   # exactly 128 bins, the most a call takes
EDGE_CASES = (
    (24, 40, 0.0, 12.0, 1, 0.25),      # every distance an integer: each kept pixel sits exactly on a bin edge; d = -8 and d = 10 are out; the
                                       # pixels at d = hi fall behind the last bin
    (40, 24, 0.5, 3.25, 0, 0.25),      # rows_are_x = 0
    (61, 97, -3.0, 100.0, 1, 0.25),    # steep line
    (1, 300, 0.02, 150.0, 0, 0.25),    # one row, the line along it 150 rows away: no pixel in range (range only, like the last case)
    (1, 300, 0.02, 150.0, 1, 0.25),    # one row, the line across it
    (300, 1, 0.1, 0.0, 1, 0.25),       # one column
    BINS_BOUND_CASE,
    (24, 40, 0.0, 12.0, 1, 18.0),      # nbin = 1
    (24, 40, 0.0, 1000.0, 1, None),    # no pixel in range; range only
)
EDGE_EMPTY_RANGE = (1e300, -1e300)     # what k_edge_dist_range stores when no pixel lies in (-8, 10)
EDGE_MAX_BINS = 128


def edge_dist(H, W, m, b, rows_are_x):
    """the expressions of metrics.slanted_edge_esf: dist = (v - m u - b) / norm, (u, v) = (row, col) if rows_are_x else (col, row)"""
    norm = np.sqrt(1 + m ** 2)
    rr, cc = np.mgrid[:H, :W]
    return ((cc - m * rr - b) / norm if rows_are_x else (rr - m * cc - b) / norm), float(norm)


@functools.lru_cache(maxsize=None)
def edge_range(case):
    """-> norm, (lo, hi) = min and max of the distances in (-8, 10), or None when there is none"""
    H, W, m, b, rows_are_x, _ = case
    dist, norm = edge_dist(H, W, m, b, rows_are_x)
    fd = dist[(dist > -8) & (dist < 10)]
    return norm, ((float(fd.min()), float(fd.max())) if fd.size else None)


def edge_bin_cases():
    return tuple(c for c in EDGE_CASES if edge_range(c)[1] is not None)


@functools.lru_cache(maxsize=None)
def edge_case(case, kind):
    """-> roi float64 [H, W]; norm, lo, hi, nbin; sums, counts float64 [nbin]: bin i holds lo + i bw <= d < lo + (i + 1) bw, found by
    searchsorted(edges, d, "right") - 1 on edges lo + i * bw; a pixel whose bin is nbin or more (d = hi on the last edge) is in none"""
    H, W, m, b, rows_are_x, bw = case
    norm, (lo, hi) = edge_range(case)
    dist, _ = edge_dist(H, W, m, b, rows_are_x)
    nbin = len(np.arange(lo, hi + bw, bw)) - 1
    edges = lo + np.arange(nbin + 1) * bw
    q = ints((H, W), kind, 7, H, W)
    fd = dist.ravel()
    keep = (fd > -8) & (fd < 10)
    which = np.searchsorted(edges, fd[keep], side="right") - 1
    ok = (which >= 0) & (which < nbin)
    tot, cnt = np.zeros(nbin, dtype=np.int64), np.zeros(nbin, dtype=np.int64)
    np.add.at(tot, which[ok], q.ravel()[keep][ok])
    np.add.at(cnt, which[ok], 1)
    return _case(roi=values(q, kind), norm=norm, lo=lo, hi=hi, nbin=nbin, sums=tot.astype(np.float64) / float(SCALE[kind]), counts=cnt.astype(np.float64),
                 dist=_ro(fd[keep]), kept=_ro(keep), dropped=int((~ok).sum()), peak=int(tot.max(initial=0)))
