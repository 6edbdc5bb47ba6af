"""Case tables, inputs and oracle references shared by tests/test_prims_edges_host.py (no GPU: the oracle against SciPy) and
tests/test_gpu_prims_edges.py (the HIP primitives against the oracle).

The cases sit where one code path of the primitives hands over to another.  What one prefilter call can be (csrc/srx_prims.hpp,
csrc/srx_fused.hpp: prefilter2d_fast):

  line kernels k_prefilter_axis0 / k_prefilter_axis1: float64 always, float32 when either side is below 64.
      n <= Horizon<T>::n (24 float, 64 double): SciPy's exact boundary sum; longer lines: the truncated sum.
      axis 0 works in chunks with Warmup<T>::n (20 / 40) warm-up samples in front and a register tail tail[WU] behind; with
      te = min(end + WU, n) - end the tail's cases are te == 0, te == 1 (cp2 falls back to prev), 0 < te < WU, te == WU with and
      without at_end.  axis 1 walks 64-column tiles with one warm-up and one tail tile; a last tile one column wide takes carry_prev
      from the tile before it.
  tile kernel k_prefilter_tile: float32 with both sides >= 64.  64 x 64 tiles with a 20-sample halo clipped at the array ends;
      walk_pass<.., 2> splits a line of n samples between two threads only when ((R+7)&~7) <= ((n-R)&~7), R = 20: from n = 44 on.  The
      last tile's region is n = (len mod 64) + 20 long (84 when len is a multiple of 64).

A zoom prefilters lines of the image's own length (MODE_MIRROR); a shift prefilters the image padded by 12 on every side
(MODE_REFLECT), so its lines are len + 24 long.

Inputs are np.rint(uniform(0, 255)) from seeded generators ("int"); the float32 runs get in addition samples with a fractional part
that float32 holds exactly ("frac"), so that the library's cast of the input is exact in both.  Every reference is computed once per
process and handed out read-only.
"""
import functools

import numpy as np

from oracle import sr_oracle as O

SEED = 459
KINDS = {"f64": ("int",), "f32": ("int", "frac")}

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the line-length cross
# ---------------------------------------------------------------------------------------------------------------------------------
# A zoom filters lines of n = L samples, a shift lines of n = L + 24.  A single image is filtered in chunks of 32 (axis 0) and segments
# of one 64-tile (axis 1); chunk k is [32 k, 32 k + 32) and its tail has te = min(32 k + 32 + WU, n) - (32 k + 32) samples.
LENGTHS = (
    # len <= 1 is copied (and k_build_taps gives every tap the index 0); 2 is the shortest line the recursion runs on; 3..5 have fewer
    # samples than the 4 taps of an output, so the mirrored / clamped tap indices fold
    1, 2, 3, 4, 5,
    # shift: n = 32, 33, 34 -- one whole chunk (te == 0), then a tail of te == 1 (cp2 falls back to prev) and of te == 2
    8, 9, 10,
    # shift: n = 40 = Warmup<double>::n, and 43, 44, 45: tails of te == 11, 12, 13 that end the line; zoom: 19, 20, 21 around Warmup<float>::n
    16, 19, 20, 21,
    # zoom: Horizon<float>::n = 24 -- SciPy's exact boundary sum up to 24, the truncated sum from 25 on
    23, 24, 25,
    # zoom: one whole chunk, and 33 = a tail of te == 1 on chunk 0 plus a last chunk of a single sample (te == 0, prev2 from the warm-up)
    31, 32, 33,
    # shift: n = 63, 64, 65 -- Horizon<double>::n = 64 (exact / truncated), the 64-tile edge of axis 1 (65: a last tile one column wide,
    # carry_prev from the tile before), and float32's hand-over from the line kernels (63) to the tile kernel (64) when the other side is 70;
    # zoom: 40 = Warmup<double>::n; 42: te == 10
    39, 40, 41, 42,
    # zoom: 57 has float's te == WU without at_end (n >= 53); 63, 64, 65 are Horizon<double>::n, the 64-tile edge and the hand-over
    # to the tile kernel; shift: n = 87, 88 -- the tile kernel's last tile region is 43, 44 long: the two-thread threshold
    57, 63, 64, 65,
    # zoom in float64: 71 -> te == 39 < WU with at_end, 72 -> te == WU with at_end, 73 -> te == WU without (and te == 9 on chunk 1);
    # shift: n = 95, 96, 97 -- three whole chunks, and a fourth of one sample behind a tail of te == 1
    71, 72, 73,
    # zoom: 87, 88 -- the two-thread threshold of the tile kernel's last tile (region 23 + 20, 24 + 20); 96, 97 as 32, 33 with warmed-up chunks in
    # front; 107, 108 end 11 / 12 samples into a chunk and 43 / 44 into a tile (shift: n = 131, 132: a third tile 3 / 4 columns wide)
    87, 88, 96, 97, 107, 108,
    # a last tile one column wide behind two, three and four whole ones (129, 193, 257); 149 = 4 * 32 + 21: float's te == WU with the line
    # ending one sample behind the tail; 289 = 9 * 32 + 1 = 4 * 64 + 33
    127, 128, 129, 149, 193, 257, 289,
    # added to the issue's list: float's te == WU WITH at_end needs n = 32 k + 20 (zoom 52, shift 28 + 24), which no length above gives
    28, 52,
)
FIXED = (9, 70)          # the other axis: 9 keeps every type on the line kernels, 70 puts float32 on the tile kernel from 64 on
CROSS_SHIFTS = ((0.37, -0.61), (-2.0, 3.0))
CROSS_ZOOMS = (1, 2)


def cross_shapes(axis):
    """The (H, W) of the cross with `axis` varied: 2 x len(LENGTHS) shapes"""
    return [((L, fixed) if axis == 0 else (fixed, L)) for fixed in FIXED for L in LENGTHS]


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. batch-driven regimes.  prefilter2d (csrc/srx_prims.hpp) sizes its launches by the batch:
#        chunk = 256; while chunk > 32 and cdiv(Wc, 64) * cdiv(Hc, chunk) * B < 4096: chunk /= 2
#        seg   = 8;   while seg > 1    and cdiv(Hc, 64) * cdiv(cdiv(Wc, 64), seg) * B < 4096: seg /= 2
#    so a single image never leaves chunk = 32, seg = 1.  Lines of 300 (5 chunks of 64, 3 of 128, 2 of 256) and of 577 (10 tiles: 5 segments
#    of 2, 3 of 4, 2 of 8; the last tile one column wide) with B = 1000 / 1500 / 2048 give chunk 64 / 128 / 256 and seg 2 / 4 / 8.  One side is
#    below 64, so float32 stays on the line kernels as well.
# ---------------------------------------------------------------------------------------------------------------------------------
BATCHES = (1000, 1500, 2048)
BATCH_CASES = {
    # name: (operation, argument, item shape, the regime the shape is there for)
    "zoom_chunk": ("zoom", 1, (300, 8), "chunk"),
    "zoom_seg": ("zoom", 1, (8, 577), "seg"),
    "shift_chunk": ("shift", (0.3, -0.2), (276, 1), "chunk"),   # Hp = 300, Wp = 25
    "shift_seg": ("shift", (0.3, -0.2), (1, 553), "seg"),       # Hp = 25, Wp = 577
}


def batch_singles(B):
    """The four items on which a batch is compared with single-item calls, bit for bit"""
    return (0, 1, B // 2, B - 1)


def cdiv(a, b):
    return -(-a // b)


def prefilter_regime(B, Hc, Wc):
    """(chunk, seg) of prefilter2d for a [B, Hc, Wc] stack: the heuristic above, restated"""
    chunk, seg = 256, 8
    while chunk > 32 and cdiv(Wc, 64) * cdiv(Hc, chunk) * B < 4096:
        chunk //= 2
    while seg > 1 and cdiv(Hc, 64) * cdiv(cdiv(Wc, 64), seg) * B < 4096:
        seg //= 2
    return chunk, seg


def batch_items(B):
    """The items of a batch that are compared with the oracle: 0..15, the last 16, every 64th in between"""
    return sorted(set(range(16)) | set(range(B - 16, B)) | set(range(0, B, 64)))


def batch_input(case, kind):
    """[max(BATCHES), h, w] float64, every item distinct; a batch of B items is its first B.  Not cached (up to 75 MB)."""
    h, w = BATCH_CASES[case][2]
    rng = np.random.default_rng([SEED, 2, sorted(BATCH_CASES).index(case)])
    x = np.rint(rng.uniform(0, 255, (max(BATCHES), h, w)))
    if kind == "frac":
        x = _fractional(x, rng)
    return x


_BATCH_REFS = {}


def batch_ref(case, kind, item, x_item):
    """The oracle on one item of batch_input(case, kind), computed once per process"""
    key = (case, kind, item)
    if key not in _BATCH_REFS:
        op, arg = BATCH_CASES[case][:2]
        O.set_threads(1)
        r = O.ndi_zoom(x_item, arg) if op == "zoom" else O.ndi_shift(x_item, arg)
        r.setflags(write=False)
        _BATCH_REFS[key] = r
    return _BATCH_REFS[key]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. blur edges: even and non-square kernels (centre at (k - 1) / 2), 1 x 1, the largest (15 x 15 = 225 of 255 taps), kernels larger
#    than the image; a width one above a 64-lane block and a height one above 16 blocks of 4 rows
# ---------------------------------------------------------------------------------------------------------------------------------
BLUR_KERNELS = ((1, 1), (2, 2), (4, 6), (3, 8), (1, 15), (15, 1), (15, 15), (7, 7))
BLUR_IMAGES = ((1, 1), (1, 7), (5, 1), (3, 5), (40, 41), (65, 129))
BLUR_BATCH = ((3, 40, 41), (4, 6))  # one batched call: [B, H, W] and the kernel's shape


@functools.lru_cache(maxsize=None)
def blur_kernel(kh, kw):
    rng = np.random.default_rng([SEED, 3, kh, kw])
    k = rng.uniform(0.05, 1.0, (kh, kw))
    k /= k.sum()
    k.setflags(write=False)
    return k


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. shift and zoom extremes, forward_model / back_project around Hp = 64
# ---------------------------------------------------------------------------------------------------------------------------------
EXTREME_IMAGES = ((1, 1), (1, 7), (5, 1), (2, 2), (24, 25), (65, 64))
EXTREME_ZOOMS = (1, 2, 3, 4)


def extreme_shifts(H, W):
    """no shift, one below every rounding, whole pixels, half pixels, and past the image (every tap index clamped)"""
    return ((0.0, 0.0), (1e-9, -1e-9), (-3.0, 2.0), (1.5, -0.5), (H + 3.2, -(W + 1.7)))


FB_HEIGHTS, FB_WIDTH = (39, 40, 41), 67          # H + 24 = 63, 64, 65 crosses the tile kernel's threshold; 39 and 41 are no multiples of f
FB_FACTORS = (2, 3)
FB_SHIFTS = ((0.37, -0.61), (1.0, -2.0))         # LR pixels: a fractional and a whole-pixel HR shift at both factors
FB_ERR_ROWS = (-1, +1)                           # back_project's err: ceil(H / f) - 1 rows (padded) and ceil(H / f) + 1 (cropped)


def fb_psf():
    from sr_mi355x import synth
    return synth.asymmetric_psf()


def fb_cases():
    """[(H, W, f, shift)]"""
    return [(H, FB_WIDTH, f, s) for H in FB_HEIGHTS for f in FB_FACTORS for s in FB_SHIFTS]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------------------
def _fractional(x, rng):
    """x plus a fractional part, rounded to float32 (exact in both precisions), kept in 0..255"""
    return np.clip(x + rng.uniform(-0.5, 0.5, x.shape), 0.0, 255.0).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def image(shape, kind="int", salt=0):
    """[H, W] float64, read-only: np.rint(uniform(0, 255)); kind "frac": plus a fractional part that float32 holds exactly"""
    rng = np.random.default_rng([SEED, 1, salt] + [int(v) for v in shape])
    x = np.rint(rng.uniform(0, 255, shape))
    if kind == "frac":
        x = _fractional(x, rng)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref(op, shape, arg, kind="int"):
    """The oracle's result of `op` on image(shape, kind), read-only.
    op: "shift" (arg: (sy, sx)), "zoom" (arg: factor), "blur" (arg: (kh, kw)), "forward" (arg: (f, shift)),
    "back" (arg: (f, shift, rows): err = image((ceil(H / f) + rows, ceil(W / f)), salt 1), shape = the HR shape)"""
    O.set_threads(1)  # images this small are slower on a team of threads
    if op == "shift":
        r = O.ndi_shift(image(shape, kind), arg)
    elif op == "zoom":
        r = O.ndi_zoom(image(shape, kind), arg)
    elif op == "blur":
        r = O.blur(image(shape, kind), blur_kernel(*arg))
    elif op == "forward":
        r = O.forward_model(image(shape, kind), fb_psf(), arg[1], arg[0])
    elif op == "back":
        r = O.back_project(back_err(shape, arg, kind), fb_psf(), arg[1], arg[0], shape)
    else:
        raise ValueError(op)
    r.setflags(write=False)
    return r


def back_err(shape, arg, kind="int"):
    """back_project's error frame for ref("back", shape, arg, kind)"""
    f, _, rows = arg
    return image((cdiv(shape[0], f) + rows, cdiv(shape[1], f)), kind, salt=1)


def worst(got, want):
    """(max |got - want|, (row, col) of it) over two arrays of one shape"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    d = np.where(np.isnan(d), np.inf, d)  # a NaN is the largest error there is
    at = np.unravel_index(int(np.argmax(d)), d.shape)
    return float(d[at]), tuple(int(v) for v in at)
