"""shift_and_add on frame sets whose frames share row offsets ("one column pass per row offset").

k_saa_tile sorts the frames by their integer row offset and runs one column pass per group of equal offsets, on the sum of the group's
row-pass images.  Every case compares S.shift_and_add_batched with the CPU oracle item by item at the primitive tolerance of the precision
(tests/test_gpu_parity.py: 5e-4 float32, 1e-9 float64), in both precisions and with the default two-pass form.  The frames are 8-bit-valued
random images, the last item of every batch has non-integer values.  The LR shapes make the 96-wide tiles of the W plane
[h f + 27, w f + 27] partial and rows != columns: 24 x 40 at x4 -> 123 x 187 (2 x 2 tiles, ragged), at x3 -> 99 x 147 (the second tile row
is 3 rows high), 56 x 88 at x2 -> 139 x 203 (2 x 3), 16 x 16 at x4 -> 91 x 91 (one tile), 16 x 24 at x4 -> 91 x 123 (1 x 2).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import sr_mi355x as S  # noqa: E402
from sr_mi355x import synth  # noqa: E402
from oracle import sr_oracle as O  # noqa: E402

PRIM_TOL = {"f64": 1e-9, "f32": 5e-4}
MAX_FRAMES = 32  # SRX_MAX_FRAMES (include/srx.h)

GRID4 = synth.phase_shifts(4)


def _shuffled(shifts, seed):
    order = np.random.default_rng(seed).permutation(len(shifts))
    return [shifts[i] for i in order]


# name -> (factor, shifts, (h, w), B)
CASES = {
    "a_grid": (4, GRID4, (24, 40), 3),                                        # four groups of four
    "b_shuffled": (4, _shuffled(GRID4, 5), (24, 40), 3),                      # groups not contiguous in the caller's order
    "c_diagonal": (4, [GRID4[5 * i] for i in range(4)], (24, 40), 2),         # every row offset distinct: groups of one
    "d_one_row": (4, GRID4[8:12], (24, 40), 2),                               # frames differing only in x: one group of four
    "e_duplicates": (4, GRID4[:7] + [GRID4[2]] + GRID4[7:] + [GRID4[13]], (24, 40), 2),  # frames equal in both offsets
    "f_nominal5": (2, synth.NOMINAL_5, (56, 88), 2),                          # groups 2 / 1 / 2, delta = 0
    "g_grid3": (3, synth.phase_shifts(3), (24, 40), 2),                       # the x3 instantiation
    "h_single": (4, [GRID4[6]], (16, 16), 2),                                 # a single frame
    "i_max_frames": (4, GRID4 * (MAX_FRAMES // 16), (16, 24), 2),             # longest groups, the geometry table full
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(f, shifts, lr [B, N, h, w] float64, oracle [B, h f, w f]): made once, shared by every test of the case, never written to."""
    f, shifts, (h, w), B = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    lr = np.round(rng.random((B, len(shifts), h, w)) * 255.0)
    lr[-1] = rng.random((len(shifts), h, w)) * 255.0  # not 8-bit-valued
    ref = np.stack([O.shift_and_add(list(lr[b]), shifts, f) for b in range(B)])
    lr.setflags(write=False)
    ref.setflags(write=False)
    return f, shifts, lr, ref


@pytest.fixture(params=["f64", "f32"])
def prec(request):
    S.set_precision(request.param)
    yield request.param
    S.set_precision("f32")


def _run(lr, shifts, f, flags=None):
    out = S.shift_and_add_batched(torch.tensor(lr), shifts, f, **({} if flags is None else {"flags": flags}))
    assert S.last_path() == "mosaic", S.last_path()  # the path k_saa_tile is on
    return out


def _check(out, ref, prec, what):
    out = out.cpu().numpy().astype(np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    for b in range(ref.shape[0]):
        d = float(np.abs(out[b] - ref[b]).max())
        print(f"{what} [{prec}] item {b}: max |delta| = {d:.3e}")
        assert d <= PRIM_TOL[prec], f"{what} item {b}: max |delta| = {d:.3e} > {PRIM_TOL[prec]:.1e}"


def test_shift_sets_have_the_groups_they_are_meant_to():
    """The row offset of a frame is floor(s_y f) up to a constant: the cases' group sizes, in ascending order of the offset."""
    def groups(name):
        f, shifts = CASES[name][:2]
        n = [int(np.floor(s[0] * f + 1e-12)) for s in shifts]
        return [n.count(v) for v in sorted(set(n))]
    assert groups("a_grid") == groups("b_shuffled") == [4, 4, 4, 4]
    assert groups("c_diagonal") == [1, 1, 1, 1]
    assert groups("d_one_row") == [4]
    assert groups("e_duplicates") == [5, 4, 4, 5]
    assert groups("f_nominal5") == [2, 1, 2]
    assert groups("g_grid3") == [3, 3, 3]
    assert groups("h_single") == [1]
    assert groups("i_max_frames") == [8, 8, 8, 8] and len(CASES["i_max_frames"][1]) == MAX_FRAMES
    a, b = CASES["a_grid"][1], CASES["b_shuffled"][1]
    assert sorted(a) == sorted(b) and a != b


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_oracle(prec, name):
    f, shifts, lr, ref = _case(name)
    _check(_run(lr, shifts, f), ref, prec, name)


def test_grid_one_pass_form(prec):
    """SRX_FLAG_DIAG_SAA_ONE_PASS: the instantiation that accumulates the halo too (k_saa_tile<T, F, false>)."""
    f, shifts, lr, ref = _case("a_grid")
    _check(_run(lr, shifts, f, flags=S.FLAG_DIAG_SAA_ONE_PASS), ref, prec, "a_grid one pass")


@pytest.mark.parametrize("name", ["a_grid", "b_shuffled"])
def test_repeatable_and_independent_of_the_batch(prec, name):
    f, shifts, lr, _ = _case(name)
    first = _run(lr, shifts, f)
    assert torch.equal(first, _run(lr, shifts, f))
    for b in range(lr.shape[0]):
        alone = _run(lr[b:b + 1], shifts, f)
        assert torch.equal(first[b], alone[0]), f"item {b} alone differs from item {b} of the batch"
