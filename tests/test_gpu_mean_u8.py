"""srx_mean_u8 / api.mean_u8: the mean over R uint8 frames of the samples at [py::f, px::f], and the session paths built on it.

The sum of at most 65535 bytes is an integer below 2^24, exact in float32 and float64, and the division by R is the only rounding, so
every comparison here is bit equality (torch.equal / np.array_equal), against two references:
  * the composition the loaders ran before: mean_frames_batched on decimate on u8_to_float, per item;
  * the integer form on the host: x.sum(axis=1, dtype=int64)[..., py::f, px::f] converted to T and divided by T(R).

The memory-contract cases register their ids through test_gpu_memory_contract.ids, as the four files of its REGISTERING_FILES do (each
id names srx_mean_u8); srx_mean_u8 takes a `void *out`, so the census of tests/test_memguard_host.py does not ask for them, and this file
is to be added to REGISTERING_FILES by a later change."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import test_gpu_memory_contract as T
import sr_mi355x as S
from sr_mi355x import _lib, api, session, synth

pytestmark = pytest.mark.gpu
CUDA = "cuda"
NP_T = {"f32": np.float32, "f64": np.float64}


def lib():
    return _lib.load()


def frames(shape, seed):
    """seeded uint8 frames with both ends of the range present"""
    a = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    a.reshape(-1)[::7] = 255
    a.reshape(-1)[3::11] = 0
    return a


def integer_ref(a, f, py, px, prec):
    """the host's integer form: [B, R, H, W] uint8 -> [B, h, w] of T"""
    t = NP_T[prec]
    return a.sum(axis=1, dtype=np.int64)[..., py::f, px::f].astype(t) / t(a.shape[1])


def composed(x, f, py, px, prec):
    """what the session ran before srx_mean_u8: u8_to_float -> decimate (per frame) -> mean_frames_batched, per item"""
    with api.precision_override(prec):
        items = []
        for b in range(x.shape[0]):
            fl = api.u8_to_float(x[b], prec)
            cut = torch.stack([api.decimate(fl[r], f, py, px) for r in range(fl.shape[0])])
            items.append(api.mean_frames_batched(cut[None])[0])
        return torch.stack(items)


def check_equal(a, f, py, px, also_composed=True):
    x = torch.from_numpy(a).to(CUDA)
    for prec in T.PRECS:
        got = S.mean_u8(x, f, py, px, precision=prec)
        want = integer_ref(a, f, py, px, prec)
        assert got.dtype == T.DT[prec] and tuple(got.shape) == want.shape
        assert np.array_equal(got.cpu().numpy(), want), (prec, a.shape, f, py, px)
        if also_composed:
            assert torch.equal(got, composed(x, f, py, px, prec)), (prec, a.shape, f, py, px)


# =====================================================================================================================================
# 1. bit equality.  (16, 64), (48, 1024): H W a multiple of 16 and rows that start aligned -- the vector forms with no head or tail;
#    (64, 259): H W a multiple of 16 with an odd W -- every row has its own head and tail; (1, 1), (5, 7), (33, 130): H W no multiple of
#    16 -- the per-sample form.  f = 3 is the per-sample form on every shape.
#    Pruning: every (shape, f, offset that fits) is run -- 9 per shape, 3 for (1, 1) -- with ONE (R, B) pair each, taken in turn from the
#    eight pairs of R in {1, 2, 5, 32} x B in {1, 3}; 9 and 8 are coprime, so over a shape the pairs rotate through f and the offsets, and over
#    the six shapes every pair meets every f.  Both precisions and both references run on each.
# =====================================================================================================================================
SHAPES = [(1, 1), (5, 7), (16, 64), (33, 130), (64, 259), (48, 1024)]
RB = list(itertools.product((1, 2, 5, 32), (1, 3)))


def _grid(shape):
    H, W = shape
    combos = [(f, py, px) for f in (1, 2, 3) for py, px in ((0, 0), (1, 0), (1, 1)) if py < H and px < W]
    k0 = SHAPES.index(shape) * 3
    return [(f, py, px) + RB[(k0 + k) % len(RB)] for k, (f, py, px) in enumerate(combos)]


def test_the_pruned_grid_still_covers_every_pairing():
    seen = {(f, R, B) for s in SHAPES for f, _, _, R, B in _grid(s)}
    assert {(f, R, B) for f in (1, 2, 3) for R, B in RB} <= seen


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_bit_equal_to_the_composition_and_to_the_integer_form(shape):
    H, W = shape
    for k, (f, py, px, R, B) in enumerate(_grid(shape)):
        check_equal(frames((B, R, H, W), 100 + k), f, py, px)


# =====================================================================================================================================
# 2. accumulator limits: a 16-bit field holds 257 frames of 255 (255 * 257 = 65535); 258 and 4096 need the 32-bit sums
# =====================================================================================================================================
@pytest.mark.parametrize("R", [256, 257, 258, 4096])
@pytest.mark.parametrize("f", [1, 2])
def test_accumulator_limits(R, f):
    H, W = 8, 48
    full = np.full((1, R, H, W), 255, dtype=np.uint8)
    x = torch.from_numpy(full).to(CUDA)
    for prec in T.PRECS:
        got = S.mean_u8(x, f, precision=prec)
        assert bool((got == 255).all()), (prec, float(got.min()), float(got.max()))
    check_equal(full, f, 0, 0, also_composed=False)
    check_equal(frames((2, R, H, W), R + f), f, 0, 0, also_composed=False)
    check_equal(frames((1, R, H, W), R + f + 9), f, 1, 1, also_composed=False)  # px = 1: rows with a head


def test_the_largest_accepted_R():
    """R = 65535: 255 * 65535 = 16711425 < 2^24 is still exact in float32.  A one-sample frame (per sample) and a 1 x 16 frame (the vector
    form, 255 groups of 257 frames), all 255 and seeded."""
    R = 65535
    for W in (1, 16):
        full = np.full((1, R, 1, W), 255, dtype=np.uint8)
        for prec in T.PRECS:
            got = S.mean_u8(torch.from_numpy(full).to(CUDA), 1, precision=prec)
            assert bool((got == 255).all()), (W, prec)
        check_equal(frames((1, R, 1, W), 7 + W), 1, 0, 0, also_composed=False)


# =====================================================================================================================================
# 2b. the grid is capped (csrc/srx_mean.hpp: 4096 blocks of 4 rows, 2 blocks of 64 lanes per item) and the lanes loop beyond it:
#     more than 16384 output rows, more than 128 vectors (vector forms) or 128 outputs (per sample) in a row
# =====================================================================================================================================
LOOP_CASES = {
    # name: ((H, W), f, py, px)
    "vec_rows_f1": ((16400, 16), 1, 0, 0),      # 16400 rows of one vector
    "vec_rows_f2": ((32808, 16), 2, 1, 1),      # 16404 output rows, a head in each
    "vec_cols_f1": ((4, 4112), 1, 0, 0),        # 257 vectors in a row: two passes and one vector of a third
    "vec_cols_f2": ((4, 4112), 2, 0, 1),
    "any_rows": ((16401, 3), 1, 0, 0),          # odd H W: per sample
    "any_cols": ((3, 401), 3, 1, 2),            # 133 outputs in a row
}


@pytest.mark.parametrize("case", list(LOOP_CASES))
def test_rows_and_columns_beyond_the_grid_cap(case):
    (H, W), f, py, px = LOOP_CASES[case]
    check_equal(frames((2, 3, H, W), 300), f, py, px, also_composed=False)


# =====================================================================================================================================
# 3. alignment: the stack 1, 2, 3 bytes past a 256-byte boundary, `out` one element past one
# =====================================================================================================================================
def _sliced(a, k):
    """`a` on the device, starting k bytes past a 256-byte boundary of a larger byte buffer"""
    raw = torch.empty(a.size + 1024, dtype=torch.uint8, device=CUDA)
    off = (-raw.data_ptr()) % 256 + k
    x = raw[off:off + a.size].view(a.shape)
    x.copy_(torch.from_numpy(a))
    assert x.data_ptr() % 256 == k
    return x


ALIGN_SHAPES = [(5, 7), (33, 131), (64, 259), (16, 80)]  # odd W and odd H W (per sample); odd W, H W % 16 == 0; all even (vector forms)


@pytest.mark.parametrize("shape", ALIGN_SHAPES, ids=[f"{h}x{w}" for h, w in ALIGN_SHAPES])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_byte_aligned_input_and_element_aligned_output(shape, k):
    H, W = shape
    B, R = 2, 3
    a = frames((B, R, H, W), 40 + k)
    x = _sliced(a, k)
    for f, prec in itertools.product((1, 2), T.PRECS):
        h, w = -(-H // f), -(-W // f)
        o = T.out((B, h, w), T.DT[prec], skip=1)
        assert o.t.data_ptr() % 256 == T.EB[prec]
        st = lib().srx_mean_u8(T.p(x), B, R, H, W, f, 0, 0, T.EB[prec], T.p(o.t), api._stream())
        torch.cuda.synchronize()
        assert st == _lib.OK
        o.check(f"{shape} f={f} {prec}")
        assert np.array_equal(o.t.cpu().numpy(), integer_ref(a, f, 0, 0, prec)), (f, prec)
        assert np.array_equal(x.cpu().numpy(), a)


# =====================================================================================================================================
# 4. memory contract: guards around `out`, every element written under every poison, the input intact
# =====================================================================================================================================
CONTRACT_CASES = {
    # name: (B, R, (H, W), f, py, px, bytes the input is off the 256-byte grid, elements the output is off it)
    "aligned_f1": (2, 5, (16, 64), 1, 0, 0, 0, 0),
    "aligned_f2": (2, 5, (16, 64), 2, 0, 0, 0, 0),
    "elem_f1": (2, 3, (64, 259), 1, 0, 0, 1, 1),      # vector form, every row with its own head and tail, scalar stores
    "elem_f2": (2, 3, (64, 259), 2, 1, 1, 3, 1),
    "oddbyte_f1": (3, 2, (33, 131), 1, 0, 0, 1, 1),   # odd H W: per sample
    "oddbyte_f2": (3, 2, (33, 131), 2, 0, 0, 3, 1),
    "oddbyte_f3": (1, 4, (5, 7), 3, 1, 2, 1, 1),
    "1x1": (1, 1, (1, 1), 2, 0, 0, 0, 0),
}
CONTRACT_IDS = [f"srx_mean_u8-{pr}-{c}" for pr in T.PRECS for c in CONTRACT_CASES]


@pytest.mark.parametrize("cid", CONTRACT_IDS, ids=T.ids(CONTRACT_IDS))
def test_memory_contract(cid):
    _, prec, case = cid.split("-")
    B, R, (H, W), f, py, px, in_skip, out_skip = CONTRACT_CASES[case]
    a = frames((B, R, H, W), 60)
    x = T.put(torch.from_numpy(a).to(CUDA), in_skip)
    assert x.data_ptr() % 256 == in_skip
    o = T.out((B, -(-(H - py) // f), -(-(W - px) // f)), T.DT[prec], out_skip)
    st = api._stream()
    res = MG.run_poisoned(lambda: lib().srx_mean_u8(T.p(x), B, R, H, W, f, py, px, T.EB[prec], T.p(o.t), st), [o], (), [x])
    assert np.array_equal(res[0].cpu().numpy(), integer_ref(a, f, py, px, prec))
    T.same(res[0], S.mean_u8(x, f, py, px, precision=prec), "srx_mean_u8")


def test_wrapper_refuses_other_dtypes_and_shapes():
    for bad in (np.zeros((1, 2, 4, 4), np.float32), np.zeros((1, 2, 4, 4), np.int16), torch.zeros((1, 2, 4, 4), dtype=torch.float64),
                torch.zeros((1, 2, 4, 4), dtype=torch.int8, device=CUDA)):
        with pytest.raises(TypeError):
            S.mean_u8(bad)
    with pytest.raises(ValueError):
        S.mean_u8(np.zeros((2, 4, 4), np.uint8))
    with pytest.raises(ValueError):
        S.mean_u8(np.zeros((1, 2, 4, 4), np.uint8), f=2, py=4)
    got = S.mean_u8(np.full((1, 2, 4, 4), 7, np.uint8), f=2)  # numpy in: uploaded as bytes, a device tensor out
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (1, 2, 2) and bool((got == 7).all())


# =====================================================================================================================================
# 5. session: rgb_cal_target combos with keep_u8, and the frame mean of a uint8 mono set
# =====================================================================================================================================
def _combo(root, counts, seed, rgb_file=None):
    """a synthetic rgb_cal_target combo: 40 x 56 raw Bayer frames, counts[k] reps of corner k, metadata.json"""
    root.mkdir(parents=True)
    base = synth.truth_image(48, 64, seed=seed)
    for c, n in enumerate(counts):
        for r in range(n):
            fr = synth.sensor_frames(np.roll(base, (c % 2, c // 2), axis=(0, 1))[4:44, 4:60], seed=seed + 8 * c + r).astype(np.uint8)
            path = str(root / f"corner{c}_rep{r:02d}.png")
            if rgb_file == (c, r):
                from PIL import Image
                Image.fromarray(np.stack([fr, fr // 2, 255 - fr], axis=2)).save(path)
            else:
                session.write_png_u8(path, fr)
    meta = {"expected_shifts": {lab: {"dy_px": dy, "dx_px": dx} for lab, (dy, dx) in zip(session.CORNER_ORDER, ((1, -1), (1, 1), (-1, -1), (-1, 1)))}}
    (root / "metadata.json").write_text(json.dumps(meta))
    return str(root)


COMBOS = {"per_corner": ((3, 3, 2, 3), None), "one_call": ((3, 3, 3, 3), None), "colour_file": ((2, 2, 2, 2), (1, 0))}


@pytest.mark.parametrize("name", list(COMBOS))
def test_rgb_cal_combo_is_the_same_with_keep_u8(tmp_path, name, monkeypatch):
    counts, rgb_file = COMBOS[name]
    combo = _combo(tmp_path / "data" / "combo", counts, 21, rgb_file)
    calls = []
    real = api.mean_u8
    monkeypatch.setattr(api, "mean_u8", lambda x, *a, **k: (calls.append(tuple(x.shape)), real(x, *a, **k))[1])
    f0, s0 = session.load_rgb_cal_combo(combo)
    assert not calls
    f1, s1 = session.load_rgb_cal_combo(combo, keep_u8=True)
    want_calls = {"per_corner": [(1, n, 40, 56) for n in counts], "one_call": [(4, 3, 40, 56)], "colour_file": []}[name]
    assert calls == want_calls
    assert s0 == s1 and len(f0) == len(f1) == 4
    for a, b in zip(f0, f1):
        assert a.dtype == b.dtype == torch.float64 and tuple(a.shape) == (20, 28) and torch.equal(a, b)
    f2, _ = session.load_session(combo, "rgb_cal_target", keep_u8=True)
    assert all(torch.equal(a, b) for a, b in zip(f0, f2))
    psf = synth.gaussian_psf()
    outs = {}
    for keep in (False, True):
        written = session.process_session(combo, psf, str(tmp_path / f"out_{int(keep)}"), kind="rgb_cal_target", n_iter=3, verbose=False, keep_u8=keep)
        assert len(written) == 1
        outs[keep] = written[0]
    names = sorted(n for n in os.listdir(outs[False]) if n.endswith((".png", ".json")))
    assert {"native_2x.png", "SAA.png", "SAA_IBP.png", "LR_red_mean.png", "convergence.json", "shifts.json"} <= set(names)
    assert names == sorted(n for n in os.listdir(outs[True]) if n.endswith((".png", ".json")))
    for fname in names:
        with open(f"{outs[False]}/{fname}", "rb") as g0, open(f"{outs[True]}/{fname}", "rb") as g1:
            assert g0.read() == g1.read(), fname


def test_reconstruct_frame_mean_of_a_uint8_set(monkeypatch):
    """a uint8 mono frame set: LR_mean and native_2x are those of the float64 set, and no float copy of the frames is made for them"""
    base = synth.truth_image(56, 72, seed=5)
    fr = [synth.sensor_frames(np.roll(base, (c % 2, c // 2), axis=(0, 1))[4:52, 4:68], seed=90 + c).astype(np.uint8) for c in range(5)]
    shifts = [s for _, s in session.IMAGE_SHIFTS]
    psf = synth.gaussian_psf()
    as_f64 = [session._to_dev_f(a) for a in fr]
    as_u8 = session._to_dev_frames(fr, keep_u8=True)
    assert all(t.dtype == torch.uint8 for t in as_u8)
    a, ea = session.reconstruct(as_f64, shifts, psf, 3)
    converted = []
    real = api.u8_to_float
    monkeypatch.setattr(api, "u8_to_float", lambda x, *p, **k: (converted.append(tuple(x.shape)), real(x, *p, **k))[1])
    b, eb = session.reconstruct(as_u8, shifts, psf, 3)
    bb = session.reconstruct_batch([as_u8, as_u8[::-1]], shifts, psf, 3)
    assert not converted
    for key in ("LR_mean", "native_2x", "SAA", "SAA_IBP"):
        assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key
        assert torch.equal(a[key], bb[0][0][key]), key
    assert a["LR_mean"].dtype == torch.float64 and ea == eb
    assert torch.equal(bb[1][0]["LR_mean"], a["LR_mean"])  # the mean does not depend on the order of the frames
