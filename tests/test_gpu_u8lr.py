"""srx_saa_u8lr_* / srx_ibp_u8lr_* / srx_decimate_u8 on the device: shift_and_add and ibp on the camera's uint8 frames (include/srx.h).

(T)uint8 is exact and every implementation either reads the frames only while it builds its tables (the mosaic family: k_mosaic_build,
k_patch_build, k_patch_near_build, the prefilter kernels of shift_and_add) or is fed a converted copy, so no tolerance appears here: a uint8
call must return the BITS of the float call on the same values -- state, MSE trace and srx_last_path() -- on every route, under the
memory contract of tests/test_gpu_memory_contract.py (guard bands, three poisons, an arena of exactly the documented size, need - 1
refused).  The float calls are held to the oracle and the reference's goldens by the other GPU tests; section 4 anchors the uint8 entry
points to the reference directly as well.

Shapes are the project's own smallest per path (T.IBP_CASES, T.SAA_CASES).  The module touches no device at import: tests/test_u8lr_host.py
imports it to register the contract ids.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as MG
import test_gpu_memory_contract as T
import test_gpu_parity as P
from conftest import load_golden
from sr_mi355x import _lib, api, session, synth
import sr_mi355x as S

pytestmark = pytest.mark.gpu

CUDA = "cuda"
DT, EB = T.DT, T.EB


def lib():
    return _lib.load()


def u8_frames(shape, seed):
    """T.rnd's integer frames as bytes, with 0 and 255 planted in every frame (first and last sample) -> uint8 [B, N, h, w] on the device"""
    x = T.rnd(shape, "f64", seed, integer=True).to(torch.uint8)
    flat = x.reshape(shape[0], shape[1], -1)
    flat[:, :, 0] = 0
    flat[:, :, -1] = 255
    return x


def path_for(prec, N, h, w, f, shp, kp, kh, kw, flags):
    return lib().srx_ibp_path_for(EB[prec], N, h, w, h * f, w * f, f, shp, kp, kh, kw, flags).decode()


# =====================================================================================================================================
# 1. every route of srx_ibp, bit for bit
# =====================================================================================================================================
IBP_U8_CASES = [c for c in T.IBP_CASES if c["integer"]]


def _ibp_id(c, tag=""):
    fl = f"-flags0x{c['flags']:x}" if c["flags"] else ""
    return f"srx_ibp_u8lr_{c['prec']}-{c['path']}-{c['name']}{tag}{fl}"


def _run_ibp(c, B=None):
    prec, f, (h, w), n_iter, flags = c["prec"], c["f"], c["hw"], c["n_iter"], c["flags"]
    B = c["B"] if B is None else B
    dt, eb, L = DT[prec], EB[prec], lib()
    N, H, W = len(c["shifts"]), h * f, w * f
    sh, shp = T.hd(c["shifts"])
    k, kp = T.hd(T._PSF[c["psf"]])
    kh, kw = k.shape
    assert path_for(prec, N, h, w, f, shp, kp, kh, kw, flags) == c["path"]
    need = L.srx_ibp_u8lr_workspace_bytes_for(eb, B, N, h, w, H, W, f, shp, kp, kh, kw, flags)
    bound = L.srx_ibp_u8lr_workspace_bytes(eb, B, N, h, w, H, W, f, flags)
    fneed = L.srx_ibp_workspace_bytes_for(eb, B, N, h, w, H, W, f, shp, kp, kh, kw, flags)
    staged = c["path"] in ("btile", "fused", "composed")
    assert 0 < need <= bound and need == fneed + (-(-(B * N * h * w * eb) // 256) * 256 if staged else 0)
    bytes_ = u8_frames((B, N, h, w), 31)
    init0 = T.rnd((B, H, W), prec, 32, integer=False)
    # the float call on the same values
    ref_hr, ref_errs = S.ibp_batched(bytes_.to(dt), sh, k, init0, f, n_iter, 0.5, precision=prec, flags=flags)
    assert S.last_path() == c["path"]
    ibp = T.fn("srx_ibp_u8lr", prec)
    for skip in (0, 1) if c["misaligned"] else (0,):  # skip = 1: the frames one BYTE off the 256-byte grid, the other pointers one element
        lr, init = T.put(bytes_, skip), T.put(init0, skip)
        assert lr.data_ptr() % 256 == skip
        hr, errs = T.out((B, H, W), dt, skip), T.out((B, n_iter), torch.float64, skip)
        call = lambda wp, wn: ibp(T.p(lr), B, N, h, w, shp, kp, kh, kw, T.p(init), H, W, f, n_iter, 0.5, T.p(hr.t), T.p(errs.t), wp, wn, api._stream(), flags)  # noqa: E731
        res = T.contract(call, [hr, errs], need, [lr, init])
        assert S.last_path() == c["path"]
        assert torch.equal(res[0], ref_hr), "state: the uint8 call differs from the float call on the same values"
        assert torch.equal(res[1], ref_errs), "MSE trace: the uint8 call differs from the float call on the same values"
        # in place (hr_out == hr_init), no trace, the arena of the shape-only bound
        buf = T.out((B, H, W), dt, skip)
        buf.preset = init.clone()
        call2 = lambda wp, wn: ibp(T.p(lr), B, N, h, w, shp, kp, kh, kw, T.p(buf.t), H, W, f, n_iter, 0.5, T.p(buf.t), None, wp, wn, api._stream(), flags)  # noqa: E731
        res2 = T.contract(call2, [buf], bound, [lr], short=False)
        assert S.last_path() == c["path"]
        assert torch.equal(res2[0], ref_hr), "in place / without the trace: a different state"


@pytest.mark.parametrize("c", IBP_U8_CASES, ids=T.ids(_ibp_id(c) for c in IBP_U8_CASES))
def test_ibp_every_route(c):
    _run_ibp(c)


def test_every_path_and_precision_is_covered():
    """the integer cases of T.IBP_CASES reach all ten names of srx_last_path() in every precision the router admits"""
    assert {(c["path"], c["prec"]) for c in IBP_U8_CASES} == {(c["path"], c["prec"]) for c in T.IBP_CASES}


# =====================================================================================================================================
# 3. instantiations the tables miss: k_mosaic_build<., 8, 1> with a ragged last group of items, the patch path's own build at B = 9
# =====================================================================================================================================
def _case(name, path, prec):
    return next(c for c in T.IBP_CASES if c["name"] == name and c["path"] == path and c["prec"] == prec)


B9_CASES = [
    dict(_case("x2_16x16", "mosaic", "f64"), misaligned=True),
    dict(_case("x2_16x16", "mosaic", "f64"), prec="f32", flags=S.FLAG_TILES, misaligned=True),  # (float32 takes a window kernel unless asked for the tiles)
    dict(_case("x4_dup", "patch", "f32"), misaligned=True),    # patch without own build: common_prep's k_mosaic_build
    dict(_case("x4_grid", "patch", "f32"), misaligned=False),  # own build (k_patch_build, k_patch_near_build)
]


@pytest.mark.parametrize("c", B9_CASES, ids=T.ids(_ibp_id(c, "-B9") for c in B9_CASES))
def test_ibp_nine_items(c):
    _run_ibp(c, B=9)


# the patch path's own build in its two read shapes (whole LR rows as 4-byte words through the LDS where the frames start on a 4-byte
# boundary; one byte per lane elsewhere -- the misaligned run of every case -- and on request), on a x4 grid, a x2 grid (LR rows of 128
# bytes, two column classes) and a 3 x 4 product grid (three row classes)
_SUB12 = [s for s in synth.phase_shifts(4) if s[0] > -0.3]
OWN_BUILD_CASES = [dict(c, flags=fl, misaligned=True)
                   for c in (_case("x4_grid", "patch", "f32"), T._from(P.PATCH_CFGS, "x2_grid", "patch", "f32"),
                             T._ibp_case("x4_sub12", "patch", "f32", 4, _SUB12, (64, 64), psf="full7", n_iter=3))
                   for fl in (0, S.FLAG_DIAG_U8_BYTE_LOADS) if not (c["name"] == "x4_grid" and fl == 0)]  # (x4_grid by default: section 1)


@pytest.mark.parametrize("c", OWN_BUILD_CASES, ids=T.ids(_ibp_id(c) for c in OWN_BUILD_CASES))
def test_ibp_patch_build_read_shapes(c):
    _run_ibp(c)


# =====================================================================================================================================
# 2. shift_and_add
# =====================================================================================================================================
SAA_U8_IDS = [(pr, c) for c, v in T.SAA_CASES.items() if c != "per_frame" for pr in v[0]]  # per_frame: frames that are not integers


def _run_saa(prec, B, f, shifts, hw, flags, path, skips, seed=21):
    (h, w), N, eb, L = hw, len(shifts), EB[prec], lib()
    sh, shp = T.hd(shifts)
    need = L.srx_saa_u8lr_workspace_bytes(eb, B, N, h, w, f)
    Bc = B if B * N <= 32768 else max(32768 // N, 1)
    assert need == L.srx_saa_workspace_bytes(eb, B, N, h, w, f) + -(-(Bc * N * h * w * eb) // 256) * 256
    bytes_ = u8_frames((B, N, h, w), seed)
    ref = S.shift_and_add_batched(bytes_.to(DT[prec]), sh, f, precision=prec, flags=flags)
    assert S.last_path() == path
    saa = T.fn("srx_saa_u8lr", prec)
    for skip in skips:
        x = T.put(bytes_, skip)
        assert x.data_ptr() % 256 == skip
        o = T.out((B, h * f, w * f), DT[prec], skip)
        call = lambda wp, wn: saa(T.p(x), B, N, h, w, shp, f, T.p(o.t), wp, wn, api._stream(), flags)  # noqa: E731
        res = T.contract(call, [o], need, [x])
        assert S.last_path() == path
        assert torch.equal(res[0], ref), "the uint8 call differs from the float call on the same values"


@pytest.mark.parametrize("prec,case", SAA_U8_IDS, ids=T.ids(f"srx_saa_u8lr_{pr}-{c}" for pr, c in SAA_U8_IDS))
def test_shift_and_add(prec, case):
    _, B, f, shifts, hw, flags, path, misaligned = T.SAA_CASES[case]
    _run_saa(prec, B, f, shifts, hw, flags, path, (0, 1) if misaligned else (0,))


PREFILTER_FORMS = {
    # name: (precision, (h, w), factor, flags): B = 3, the frames one byte off the grid
    "k_prefilter_64": ("f32", (64, 64), 4, 0),
    "k_prefilter_small_f32": ("f32", (41, 57), 3, 0),   # odd h w: every other frame starts on an odd byte
    "k_prefilter_small_f64": ("f64", (41, 57), 3, 0),
    "tile_kernel_f32": ("f32", (72, 140), 2, 0),        # float32 planes of at least 64 x 64 go through k_prefilter_tile by default ...
    "line_kernels_f32": ("f32", (72, 140), 2, S.FLAG_DIAG_NO_PREFILTER_TILE),  # ... and through the line kernels on request,
    "line_kernels_f64": ("f64", (72, 140), 2, 0),       # as float64 always does
}


@pytest.mark.parametrize("form", list(PREFILTER_FORMS), ids=T.ids(f"srx_saa_u8lr_{PREFILTER_FORMS[n][0]}-{n}" for n in PREFILTER_FORMS))
def test_shift_and_add_prefilter_forms(form):
    prec, hw, f, flags = PREFILTER_FORMS[form]
    _run_saa(prec, 3, f, synth.phase_shifts(f), hw, flags, "mosaic", (1,), seed=22)


# =====================================================================================================================================
# 4. anchor to the reference: the goldens' own uint8 arrays through the wrappers
# =====================================================================================================================================
def _anchors():
    c1, c2 = load_golden("synth_c1.npz"), load_golden("synth_c2_small.npz")
    return {
        # name: (lr uint8, shifts, psf, factor, golden SAA or None, {n: golden IBP}, golden trace or None)
        "c1_lr_nom": (c1["lr_nom"], c1["shifts_nom"], c1["psf_g"], 2, c1["saa_nom"], {n: c1[f"ibp_nom_{n}"] for n in (1, 2, 10)}, c1["ibp_nom_errors"]),
        # (the goldens' "meas" reconstructions are of the rep AVERAGE; for the stored uint8 lr_meas itself the reference is its CPU port,
        #  oracle/sr_oracle.py, which tests/test_oracle_golden.py holds to the same goldens)
        "c1_lr_meas": (c1["lr_meas"], c1["shifts_meas"], c1["psf_m"], 2, None, {}, None),
        "c2_lr16": (c2["lr16"], c2["shifts16"], c2["psf_g"], 4, c2["saa16"], {n: c2[f"ibp16_{n}"] for n in (1, 10)}, c2["ibp16_errors"]),
        "c2_lr4": (c2["lr4"], c2["shifts4"], c2["psf_m"], 4, c2["saa4"], {n: c2[f"ibp4_{n}"] for n in (1, 10)}, c2["ibp4_errors"]),
    }


ANCHOR_NAMES = ("c1_lr_nom", "c1_lr_meas", "c2_lr16", "c2_lr4")


@pytest.fixture(scope="module")
def anchors():
    """per anchor: the frames and, computed ONCE, the references at 1, 2 and 10 iterations -- the golden where the reference stored one, the
    oracle (the reference's loop, continued from nothing else than the same inputs) where it did not"""
    from oracle import sr_oracle as O
    out = {}
    for name, (lr, shifts, psf, f, g_saa, g_ibp, g_err) in _anchors().items():
        assert lr.dtype == np.uint8
        frames = [a.astype(np.float64) for a in lr]
        saa = g_saa if g_saa is not None else O.shift_and_add(frames, shifts, f)
        refs, errs = dict(g_ibp), g_err
        if any(n not in refs for n in (1, 2, 10)):
            for n in (1, 2, 10):
                if n not in refs:
                    refs[n], e = O.ibp(frames, shifts, psf, saa, f, n, 0.5)
                    if errs is None and n == 10:
                        errs = np.asarray(e)
        out[name] = (lr, shifts, psf, f, saa, refs, np.asarray(errs))
    return out


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("name", ANCHOR_NAMES)
def test_anchor_to_the_reference(anchors, name, prec):
    lr, shifts, psf, f, saa_ref, refs, errs_ref = anchors[name]
    lr_u8 = torch.from_numpy(lr)[None]
    saa = S.shift_and_add_u8_batched(lr_u8, shifts, f, precision=prec)
    P.close(saa[0].cpu().numpy(), saa_ref, P.PRIM_TOL[prec])
    for n in (1, 2, 10):
        hr, errs = S.ibp_u8_batched(lr_u8, shifts, psf, saa_ref[None], f, n, 0.5, precision=prec)
        d = float(np.abs(hr[0].cpu().numpy().astype(np.float64) - refs[n]).max())
        print(f"{name} {prec} n_iter={n}: max |hr - reference| = {d:.3e} (path {S.last_path()})")
        P.close(hr[0].cpu().numpy(), refs[n], P.IBP_TOL[prec])
        np.testing.assert_allclose(errs[0].cpu().numpy(), errs_ref[:n], rtol=P.ERR_RTOL[prec])


# =====================================================================================================================================
# 5. srx_decimate_u8
# =====================================================================================================================================
DECIMATE_CASES = {
    # name: (B, (H, W), f, py, px)
    "37x50": (1, (37, 50), 2, 0, 0),   # extract_red of a raw Bayer frame
    "5x7": (3, (5, 7), 3, 1, 2),
    "1x1": (1, (1, 1), 2, 0, 0),
}


@pytest.mark.parametrize("case", list(DECIMATE_CASES), ids=T.ids(f"srx_decimate_u8-{c}" for c in DECIMATE_CASES))
def test_decimate_u8(case):
    B, (H, W), f, py, px = DECIMATE_CASES[case]
    a = np.random.default_rng(51).integers(0, 256, (B, H, W), dtype=np.uint8)
    want = a[:, py::f, px::f]
    for skip in (0, 1):  # skip = 1: an odd base pointer, in and out
        x, o = T.put(torch.from_numpy(a).to(CUDA), skip), T.out(want.shape, torch.uint8, skip)
        assert x.data_ptr() % 2 == skip
        res = MG.run_poisoned(lambda: lib().srx_decimate_u8(T.p(x), B, H, W, f, py, px, T.p(o.t), api._stream()), [o], (), [x], MG.INT_POISONS)
        assert np.array_equal(res[0].cpu().numpy(), want)
    assert np.array_equal(S.decimate_u8(a, f, py, px), want)
    assert np.array_equal(S.decimate_u8(torch.from_numpy(a[0]).to(CUDA), f, py, px).cpu().numpy(), want[0])
    if (f, py, px) == (2, 0, 0):
        assert np.array_equal(S.extract_red_u8(a[0]), a[0, 0::2, 0::2])


# =====================================================================================================================================
# 6. wrappers and session drivers
# =====================================================================================================================================
def test_wrappers_refuse_other_dtypes():
    sh, k = synth.NOMINAL_4, synth.gaussian_psf()
    init = np.zeros((1, 32, 32))
    for bad in (np.zeros((1, 4, 16, 16), np.float32), np.zeros((1, 4, 16, 16), np.int16), torch.zeros((1, 4, 16, 16), dtype=torch.float64),
                torch.zeros((1, 4, 16, 16), dtype=torch.int8, device=CUDA)):
        with pytest.raises(TypeError):
            S.shift_and_add_u8_batched(bad, sh, 2)
        with pytest.raises(TypeError):
            S.ibp_u8_batched(bad, sh, k, init, 2, 1)
    with pytest.raises(TypeError):
        S.decimate_u8(np.zeros((4, 4), np.float64), 2)


def _barcode_frames(reps, shape=(48, 64), seed=77):
    """reps x 4 uint8 frames: shifted crops of one seeded image, each with its own sensor noise"""
    base = synth.truth_image(shape[0] + 8, shape[1] + 8, seed=seed)
    return [[synth.sensor_frames(np.roll(base, (c % 2 + r, c // 2), axis=(0, 1))[4:4 + shape[0], 4:4 + shape[1]], seed=seed + 4 * r + c).astype(np.uint8)
             for c in range(4)] for r in range(reps)]


def test_reconstruct_batch_on_uint8_frames():
    """two reps of four uint8 48 x 64 frames: tensor for tensor what the float64-loaded frames give"""
    reps = _barcode_frames(2)
    psf = synth.gaussian_psf()
    as_f64 = [[session._to_dev_f(a) for a in fr] for fr in reps]
    as_u8 = [session._to_dev_frames(fr, keep_u8=True) for fr in reps]
    assert all(t.dtype == torch.uint8 for fr in as_u8 for t in fr) and all(t.dtype == torch.float64 for fr in as_f64 for t in fr)
    for prec in T.PRECS:
        S.set_precision(prec)
        try:
            a = session.reconstruct_batch(as_f64, session.CORNER_SHIFTS, psf, 5)
            b = session.reconstruct_batch(as_u8, session.CORNER_SHIFTS, psf, 5)
            one = session.reconstruct(as_u8[1], session.CORNER_SHIFTS, psf, 5)
        finally:
            S.set_precision("f32")
        for (ia, ea), (ib, eb) in zip(a, b):
            assert ea == eb
            for key in ("native_2x", "SAA", "SAA_IBP", "LR_mean"):
                assert ia[key].dtype == ib[key].dtype and torch.equal(ia[key], ib[key]), (prec, key)
        assert one[1] == a[1][1] and all(torch.equal(one[0][key], a[1][0][key]) for key in one[0])


@pytest.mark.parametrize("red", [False, True], ids=["mono_barcodes", "rgb_barcodes"])
def test_session_files_are_the_same_with_keep_u8(tmp_path, red):
    from PIL import Image
    shape = (96, 128) if red else (48, 64)
    sess = tmp_path / "data" / "bc"
    sess.mkdir(parents=True)
    for r, fr in enumerate(_barcode_frames(2, shape)):
        for c, a in enumerate(fr):
            Image.fromarray(a).save(sess / f"corner{c}_rep{r:02d}.png")
    kind = "rgb_barcodes" if red else "mono_barcodes"
    psf = synth.gaussian_psf()
    outs = {}
    for keep in (False, True):
        base = tmp_path / f"out_{int(keep)}"
        written = session.process_session(str(sess), psf, str(base), kind=kind, n_iter=5, verbose=False, keep_u8=keep)
        assert len(written) == 2
        outs[keep] = written
    for d0, d1 in zip(outs[False], outs[True]):
        for fname in ("native_2x.png", "SAA.png", "SAA_IBP.png", "LR_red_mean.png" if red else "LR_mean.png", "convergence.json"):
            with open(f"{d0}/{fname}", "rb") as f0, open(f"{d1}/{fname}", "rb") as f1:
                assert f0.read() == f1.read(), fname


# ---------------------------------------------------------------------------------------------------------------------------------
CONTRACT = ([_ibp_id(c) for c in IBP_U8_CASES] + [_ibp_id(c, "-B9") for c in B9_CASES] + [_ibp_id(c) for c in OWN_BUILD_CASES] + [f"srx_saa_u8lr_{pr}-{c}" for pr, c in SAA_U8_IDS]
            + [f"srx_saa_u8lr_{PREFILTER_FORMS[n][0]}-{n}" for n in PREFILTER_FORMS] + [f"srx_decimate_u8-{c}" for c in DECIMATE_CASES])
