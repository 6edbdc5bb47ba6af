"""srx_patches_* and sr_mi355x.patchwise without a GPU.

1. The argument checks and refusals of the gather and blend entry points (decided on the host before any HIP call: the pointers are never
   dereferenced) and srx_patches_count against the reference's grid rule.
2. Properties of the rule on the numpy reference (tests/patchwise_cases.py): the weight sum is positive everywhere, at most three
   patches per axis cover a sample, S <= 2 R.
3. tests/patchwise_host_model.cpp -- the __host__ __device__ grid / weight / blend functions of csrc/srx_patches.hpp in a host loop, built
   with g++ -fsanitize=address,undefined: its output equals the numpy reference bit for bit and no sanitizer report appears.
4. PatchGrid and the command line's refusals."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import patchwise_cases as PC
from sr_mi355x import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "enph459-super-resolution_amd", "csrc")
GXX = shutil.which("g++")
FAKE = ctypes.c_void_p(4096)

GATHER = ("srx_patches_gather_u8", "srx_patches_gather_f32", "srx_patches_gather_f64")
BLEND = ("srx_patches_blend_f32", "srx_patches_blend_f64")
G_OK = dict(src=FAKE, B=2, N=3, h=150, w=171, ph=64, pw=64, sy=48, sx=48, out=FAKE)
B_OK = dict(src=FAKE, B=1, H=300, W=342, PH=128, PW=128, SY=96, SX=96, margin=8, out=FAKE)


def gather(entry, **kw):
    a = dict(G_OK, **kw)
    return getattr(_lib.load(), entry)(a["src"], a["B"], a["N"], a["h"], a["w"], a["ph"], a["pw"], a["sy"], a["sx"], a["out"], None)


def blend(entry, **kw):
    a = dict(B_OK, **kw)
    return getattr(_lib.load(), entry)(a["src"], a["B"], a["H"], a["W"], a["PH"], a["PW"], a["SY"], a["SX"], a["margin"], a["out"], None)


G_INVALID = {"null_frames": dict(src=None), "null_out": dict(out=None), "B0": dict(B=0), "B_neg": dict(B=-2), "N0": dict(N=0), "h0": dict(h=0),
             "w_neg": dict(w=-171), "ph0": dict(ph=0), "ph_over_h": dict(ph=151), "pw_neg": dict(pw=-1), "pw_over_w": dict(pw=172),
             "sy0": dict(sy=0), "sy_over_ph": dict(sy=65), "sx_neg": dict(sx=-48), "sx_over_pw": dict(sx=65)}
G_UNSUPPORTED = {"2sy_below_ph": dict(sy=31), "2sx_below_pw": dict(sx=31),
                 "item_2GiB": dict(N=8, h=1 << 14, w=1 << 14, ph=1 << 14, pw=1 << 14, sy=1 << 14, sx=1 << 14),   # 2^31 samples of any type
                 "plane_over_int": dict(N=1, h=1 << 16, w=1 << 16),
                 "BP_over_int": dict(B=1 << 30, N=1, h=4, w=4, ph=2, pw=2, sy=1, sx=1)}                          # P = 9


@pytest.mark.parametrize("entry", GATHER)
def test_gather_refusals(entry):
    for name, kw in G_INVALID.items():
        assert gather(entry, **kw) == _lib.E_INVALID, name
    for name, kw in G_UNSUPPORTED.items():
        assert gather(entry, **kw) == _lib.E_UNSUPPORTED, name
    assert gather(entry, sy=31, B=0) == _lib.E_INVALID        # invalid wins over unsupported
    assert gather(entry, sy=31, sx=65) == _lib.E_INVALID


def test_gather_2gib_rule_counts_bytes():
    """one item's frames of 2 GiB or more: 2^29 samples pass as uint8 and float32 (2 GiB exactly: refused) by their bytes"""
    big = dict(N=2, h=1 << 14, w=1 << 14, ph=64, pw=64, sy=48, sx=48)   # 2^29 samples
    assert gather("srx_patches_gather_f32", **big) == _lib.E_UNSUPPORTED
    assert gather("srx_patches_gather_f64", **big) == _lib.E_UNSUPPORTED
    assert gather("srx_patches_gather_u8", **dict(big, N=8)) == _lib.E_UNSUPPORTED
    assert gather("srx_patches_gather_u8", **dict(big, src=None)) == _lib.E_INVALID  # (below the limit as bytes: only the null pointer refuses it)


B_INVALID = {"null_patches": dict(src=None), "null_out": dict(out=None), "B0": dict(B=0), "H0": dict(H=0), "W_neg": dict(W=-342),
             "PH0": dict(PH=0), "PH_over_H": dict(PH=301), "PW_over_W": dict(PW=343), "SY0": dict(SY=0), "SY_over_PH": dict(SY=129),
             "SX_over_PW": dict(SX=129), "margin_neg": dict(margin=-1), "R0_rows": dict(margin=16), "R0_no_overlap": dict(SY=128, margin=0),
             "R_neg_cols": dict(SX=120, margin=8)}
B_UNSUPPORTED = {"2SY_below_PH": dict(SY=63, margin=0), "2SX_below_PW": dict(SX=63, margin=0),
                 "plane_2GiB_f64": dict(H=1 << 14, W=1 << 14), "plane_over_int": dict(H=1 << 16, W=1 << 16),
                 "BP_over_int": dict(B=1 << 30, H=4, W=4, PH=2, PW=2, SY=1, SX=1, margin=0)}


@pytest.mark.parametrize("entry", BLEND)
def test_blend_refusals(entry):
    for name, kw in B_INVALID.items():
        assert blend(entry, **kw) == _lib.E_INVALID, name
    for name, kw in B_UNSUPPORTED.items():
        if name == "plane_2GiB_f64" and entry.endswith("f32"):
            continue  # 2^28 float32 samples are 1 GiB
        assert blend(entry, **kw) == _lib.E_UNSUPPORTED, name
    assert blend(entry, SY=63, margin=40) == _lib.E_INVALID   # R < 1 (invalid) wins over 2 s < L (unsupported)


def test_count_is_the_grid_rule():
    lib = _lib.load()
    for n in (1, 2, 5, 64, 65, 97, 150, 171, 300, 342, 1536, 2048, 4096):
        for L in (1, 2, 3, 32, 64, 128, 256):
            for s in range(1, L + 1, max(1, L // 7)):
                want = PC.count(n, L, s) if PC.accepted(n, L, s) else 0
                assert lib.srx_patches_count(n, L, s) == want, (n, L, s)
    assert lib.srx_patches_count(1536, 128, 112) == 14 and lib.srx_patches_count(2048, 128, 112) == 19  # the default grid: 266 patches
    for bad in ((0, 4, 2), (-5, 4, 2), (8, 0, 2), (8, 9, 5), (8, 4, 0), (8, 4, 5), (8, 4, 1), (8, -4, -2)):
        assert lib.srx_patches_count(*bad) == 0, bad
    assert lib.srx_patches_count((1 << 31) - 1, 2, 1) == (1 << 31) - 2


def test_symbols_are_in_the_ctypes_table():
    assert set(GATHER) | set(BLEND) | {"srx_patches_count"} <= set(_lib.symbols())


# ---------------------------------------------------------------------------------------------------------------------------------
# properties of the rule, on the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def test_weight_sums_are_positive_and_cover_is_at_most_three():
    checked = 0
    for L in (2, 3, 4, 7, 16, 33):
        for s in range((L + 1) // 2, L + 1):
            for margin in range(0, L):
                R = L - s - 2 * margin
                if R < 1:
                    break
                for n in sorted({L, L + 1, L + s - 1, L + s, L + s + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 2, 5 * L + 3, 4 * s + L, 4 * s + L + 1}):
                    S, cover = PC.weight_sums(n, L, s, margin)
                    assert S.min() >= 1 and S.max() <= 2 * R, (n, L, s, margin, S.min(), S.max())
                    assert 1 <= cover.min() and cover.max() <= 3, (n, L, s, margin)
                    o = PC.origins(n, L, s)
                    assert o[0] == 0 and o[-1] == n - L and all(b > a for a, b in zip(o, o[1:])), (n, L, s)
                    checked += 1
    assert checked > 1000
    _, cover = PC.weight_sums(65, 32, 16, 0)
    assert cover.max() == 3  # n = 2 L + 1 at s = L / 2: the case the GPU test runs


# ---------------------------------------------------------------------------------------------------------------------------------
# the host model under the sanitizers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if GXX is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("patchwise_model") / "patchwise_host_model")
    subprocess.check_call([GXX, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "patchwise_host_model.cpp")])
    return exe


@pytest.mark.parametrize("kind", ("f32", "f64"))
@pytest.mark.parametrize("name", list(PC.BLEND_CASES))
def test_model_blend_is_the_reference_bit_for_bit(model, tmp_path, name, kind):
    B, H, W, PH, PW, SY, SX, margin = PC.BLEND_CASES[name]
    dt = np.float32 if kind == "f32" else np.float64
    patches = PC.blend_case(name, dt)
    src, dst = str(tmp_path / "patches.bin"), str(tmp_path / "out.bin")
    patches.tofile(src)
    r = subprocess.run([model, kind] + [str(v) for v in (B, H, W, PH, PW, SY, SX, margin)] + [src, dst], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr[-3000:]}"
    words = [int(v) for v in r.stdout.split()]
    oy, ox = PC.origins(H, PH, SY), PC.origins(W, PW, SX)
    assert words == [len(oy), len(ox)] + oy + ox
    got = np.fromfile(dst, dtype=dt).reshape(B, H, W)
    want = PC.blend(patches, H, W, SY, SX, margin)
    assert want.dtype == dt and np.array_equal(got.view(np.uint8), want.view(np.uint8))
    slack = 8 * np.finfo(dt).eps * np.abs(patches).max()  # a convex combination, up to the roundings of at most nine terms and one division
    assert np.isfinite(want).all() and want.min() >= patches.min() - slack and want.max() <= patches.max() + slack


def test_reference_round_trip_is_exact_for_bytes():
    """blend(gather(img)) == img for integer images in 0..255: every partial sum is an integer below 2^24 (S <= 2 R per axis)"""
    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, (1, 1, 150, 171)).astype(np.float32)
    p = PC.gather(img, 64, 64, 48, 48)[:, 0]
    for margin in (0, 7):
        assert np.array_equal(PC.blend(p, 150, 171, 48, 48, margin)[0], img[0, 0])


# ---------------------------------------------------------------------------------------------------------------------------------
# PatchGrid, the command line
# ---------------------------------------------------------------------------------------------------------------------------------
def test_patch_grid():
    from sr_mi355x import patchwise
    g = patchwise.PatchGrid(1536, 2048, 2)
    assert (g.patch_lr, g.s_lr, g.L_hr, g.s_hr, g.gy, g.gx, g.P) == (128, 112, 256, 224, 14, 19, 266)
    assert g.oy_lr.tolist() == PC.origins(1536, 128, 112) and g.ox_lr.tolist() == PC.origins(2048, 128, 112)
    assert g.oy_hr.tolist() == PC.origins(3072, 256, 224) and g.ox_hr.tolist() == PC.origins(4096, 256, 224)  # the HR grid is the LR grid times f
    assert g.centres_lr.shape == (14, 19, 2) and g.centres_lr[0, 0].tolist() == [63.5, 63.5] and g.centres_hr[0, 0].tolist() == [127.5, 127.5]
    assert g.centres_lr[-1, -1].tolist() == [1536 - 64.5, 2048 - 64.5]
    g3 = patchwise.PatchGrid(96, 112, 3, patch_lr=64, overlap_lr=32, margin_hr=4)
    assert (g3.L_hr, g3.s_hr, g3.gy, g3.gx) == (192, 96, 2, 3)
    for bad in (dict(patch_lr=200), dict(patch_lr=64, overlap_lr=40), dict(patch_lr=64, overlap_lr=-1), dict(patch_lr=64, overlap_lr=16, margin_hr=16),
                dict(patch_lr=64, overlap_lr=0), dict(patch_lr=64, margin_hr=-1)):
        with pytest.raises(ValueError):
            patchwise.PatchGrid(96, 112, 2, **bad)
    import sr_mi355x
    assert sr_mi355x.PatchGrid is patchwise.PatchGrid and sr_mi355x.reconstruct_patchwise is patchwise.reconstruct_patchwise
    assert sr_mi355x.estimate_shift_field is patchwise.estimate_shift_field


def test_run_sr_refuses_patchwise_with_row_bands(tmp_path, capsys):
    from sr_mi355x import run_sr
    base = ["--kind", "mono_cal_target", "--data-dir", str(tmp_path), "--output-dir", str(tmp_path / "out")]
    for extra in (["--patchwise", "local", "--row-bands"], ["--patchwise", "global", "--row-bands"], ["--patchwise", "sometimes"]):
        with pytest.raises(SystemExit) as e:
            run_sr.main(base + extra)
        assert e.value.code == 2
    assert "--patchwise" in capsys.readouterr().err
