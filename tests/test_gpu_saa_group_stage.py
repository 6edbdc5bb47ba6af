"""shift_and_add with the row passes of a group staged in chunks ("the staged row pass").

k_saa_tile<float, 4, true, G> stores the LR patches of up to G frames of a row-offset group into LDS slots of their own, runs their row
passes back to back behind one barrier, and stages the next chunk into a second set of slots meanwhile.  What can go wrong is the
bookkeeping of that staging: a chunk shorter than G at a group's end, a short chunk followed by a long one (at the shipped G = 2 the frame
staged under the short chunk's row pass and the one under its column pass fill the long one; the staging loop at a chunk's turn then runs for the
first chunk of a tile only), the slot sets changing hands, frames of different x offsets side by side in one set.  So the frame sets run every chunk
remainder for G = 2 and 4 in one group (1, 2, 3, 4, 5, 7, 8, 9 frames), eight full chunks with the geometry table full (32 frames), uneven
groups (5 / 4 / 4 / 5), groups of one, and the 16 phases in shuffled order; on one tile (16 x 16 at x4 -> a 91 x 91 plane), on 2 x 2 ragged
tiles (24 x 40 -> 123 x 187) and on the flagship's 3 x 3 tiles with the 91-wide last one (64 x 64 -> 283 x 283, B = 2).

Every case compares S.shift_and_add_batched with the CPU oracle item by item at tests/test_gpu_saa_groups.py's tolerances (5e-4 float32,
1e-9 float64), in both precisions: float64 runs the per-frame instantiation (G = 1) that must be untouched.  The frames are 8-bit-valued,
the last item of a batch is not.  Each batch runs twice and must give equal bits, and every item run alone must equal its item of the
batch bit for bit.  One case per shape writes into an output pre-filled with NaN.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sr_mi355x as S  # noqa: E402
from sr_mi355x import _lib, api, synth  # noqa: E402
from oracle import sr_oracle as O  # noqa: E402

PRIM_TOL = {"f64": 1e-9, "f32": 5e-4}
MAX_FRAMES = 32  # SRX_MAX_FRAMES (include/srx.h)
F = 4

GRID4 = synth.phase_shifts(4)
ROW = GRID4[4:8]  # one row offset, four column offsets


def _shuffled(shifts, seed):
    order = np.random.default_rng(seed).permutation(len(shifts))
    return [shifts[i] for i in order]


# name -> shifts
SETS = {f"one_row_{n}": [ROW[(3 * i) % 4] for i in range(n)] for n in (1, 2, 3, 4, 5, 7, 8, 9)}  # x offsets 0, 3, 2, 1, 0, ...: neighbours differ
SETS.update({
    "one_row_32": ROW * (MAX_FRAMES // 4),                               # eight full chunks of four, geo[] full
    "uneven_5445": GRID4[:7] + [GRID4[2]] + GRID4[7:] + [GRID4[13]],     # chunks 4 + 1 | 4 | 4 | 4 + 1 at G = 4
    "groups_of_one": [GRID4[5 * i] for i in range(4)],                   # every chunk a single frame
    "grid_shuffled": _shuffled(GRID4, 11),                               # four groups of four, not contiguous in the caller's order
})
# name -> ((h, w), B)
SHAPES = {"one_tile": ((16, 16), 2), "ragged_2x2": ((24, 40), 2), "flagship_3x3": ((64, 64), 2)}
CASES = [(sh, st) for sh in SHAPES for st in SETS]


@functools.lru_cache(maxsize=None)
def _case(shape, frames):
    """(shifts, lr [B, N, h, w] float64, oracle [B, h f, w f]): made once, shared by every test of the case, never written to."""
    (h, w), B = SHAPES[shape]
    shifts = SETS[frames]
    rng = np.random.default_rng(1000 * sorted(SHAPES).index(shape) + sorted(SETS).index(frames))
    lr = np.round(rng.random((B, len(shifts), h, w)) * 255.0)
    lr[-1] = rng.random((len(shifts), h, w)) * 255.0  # not 8-bit-valued
    ref = np.stack([O.shift_and_add(list(lr[b]), shifts, F) for b in range(B)])
    lr.setflags(write=False)
    ref.setflags(write=False)
    return shifts, lr, ref


@pytest.fixture(params=["f64", "f32"])
def prec(request):
    S.set_precision(request.param)
    yield request.param
    S.set_precision("f32")


def _run(lr, shifts):
    out = S.shift_and_add_batched(torch.tensor(lr), shifts, F)
    assert S.last_path() == "mosaic", S.last_path()  # the path k_saa_tile is on
    return out


def _check(out, ref, prec, what):
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    for b in range(ref.shape[0]):
        d = float(np.abs(out[b] - ref[b]).max())
        print(f"{what} [{prec}] item {b}: max |delta| = {d:.3e}")
        assert d <= PRIM_TOL[prec], f"{what} item {b}: max |delta| = {d:.3e} > {PRIM_TOL[prec]:.1e}"


def test_frame_sets_have_the_groups_they_are_meant_to():
    """The row offset of a frame is floor(s_y f) up to a constant: the sets' group sizes, in ascending order of the offset.  (No GPU.)"""
    def groups(name):
        n = [int(np.floor(s[0] * F + 1e-12)) for s in SETS[name]]
        return [n.count(v) for v in sorted(set(n))]
    for n in (1, 2, 3, 4, 5, 7, 8, 9):
        assert groups(f"one_row_{n}") == [n]
        xs = [s[1] for s in SETS[f"one_row_{n}"]]
        assert all(a != b for a, b in zip(xs, xs[1:]))  # neighbours in a chunk have different column offsets
    assert groups("one_row_32") == [MAX_FRAMES] and len(SETS["one_row_32"]) == MAX_FRAMES
    assert groups("uneven_5445") == [5, 4, 4, 5]
    assert groups("groups_of_one") == [1, 1, 1, 1]
    assert groups("grid_shuffled") == [4, 4, 4, 4]
    assert sorted(SETS["grid_shuffled"]) == sorted(GRID4) and SETS["grid_shuffled"] != GRID4
    # every remainder of a group's length by the chunk lengths 2 and 4 occurs among the one-row sets
    assert {n % 2 for n in (1, 2, 3, 4, 5, 7, 8, 9)} == {0, 1} and {n % 4 for n in (1, 2, 3, 4, 5, 7, 8, 9)} == {0, 1, 2, 3}
    # the W plane [h f + 27, w f + 27] in 96-wide tiles: 1 x 1, 2 x 2 ragged, 3 x 3 with a 91-wide last tile
    tiles = {k: tuple(-(-(v * F + 27) // 96) for v in hw) for k, (hw, _) in SHAPES.items()}
    assert tiles == {"one_tile": (1, 1), "ragged_2x2": (2, 2), "flagship_3x3": (3, 3)}
    assert (64 * F + 27) - 2 * 96 == 91


@pytest.mark.gpu
@pytest.mark.parametrize("shape,frames", CASES)
def test_against_the_oracle(prec, shape, frames):
    shifts, lr, ref = _case(shape, frames)
    _check(_run(lr, shifts), ref, prec, f"{shape} {frames}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,frames", CASES)
def test_repeatable_and_independent_of_the_batch(prec, shape, frames):
    shifts, lr, _ = _case(shape, frames)
    first = _run(lr, shifts)
    assert torch.equal(first, _run(lr, shifts)), "two runs of one batch differ"
    for b in range(lr.shape[0]):
        alone = _run(lr[b:b + 1], shifts)
        assert torch.equal(first[b], alone[0]), f"item {b} alone differs from item {b} of the batch"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_output_prefilled_with_nan(prec, shape):
    """srx_saa through the C entry point into an output full of NaN: every element is stored, and with the bits of the ordinary call."""
    shifts, lr, ref = _case(shape, "uneven_5445")
    B, N, h, w = lr.shape
    x = api._to_dev(torch.tensor(lr), prec)[0]
    sh, shp, per_item = api._shift_tables(shifts, B, N)
    assert not per_item
    out = torch.full((B, h * F, w * F), float("nan"), dtype=api._TORCH_DT[prec], device=x.device)
    wt, wp, wn = api._ws(_lib.load().srx_saa_workspace_bytes(api._ELEM[prec], B, N, h, w, F))
    _lib.check(api._fn("srx_saa", prec)(api._p(x), B, N, h, w, shp, F, api._p(out), wp, wn, api._stream(), 0), "srx_saa")
    torch.cuda.synchronize()
    assert S.last_path() == "mosaic", S.last_path()
    assert not bool(torch.isnan(out).any()), "an element of the output was not stored"
    _check(out, ref, prec, f"{shape} uneven_5445 into NaN")
    assert torch.equal(out, _run(lr, shifts))
