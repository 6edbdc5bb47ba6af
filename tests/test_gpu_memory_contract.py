"""The memory contract of include/srx.h, entry point by entry point: a call writes its outputs and bytes [0, ws_bytes) of its workspace and
nothing else, depends on nothing the workspace or the outputs held before, leaves its inputs alone, and refuses a short workspace on the
host.  tests/memguard.py explains why buffers from torch.empty cannot show a violation of any of this and what is used instead (guard
bands around exact-size payloads, three poisons, bit-identity across poisons).

Calls go through the C ABI (sr_mi355x.api allocates its own buffers).  Every case also runs once through the sr_mi355x wrapper and must
be bit-identical to it, so the values inherit the oracle parity the other GPU tests establish for the same configurations; no tolerance
appears in this file.  Every test id names the entry points it calls (tests/test_memguard_host.py compares them with include/srx.h), and
every srx_ibp case asserts the path it is there for.

Pointer alignment (srx.h): the workspace on the 256-byte grid, checked on the host; image, output and errors pointers need their element
type's alignment only -- no kernel casts a caller pointer to a vector type (arena planes alone move as 16-byte vectors; k_ibp_patch's
128-bit buffer stores into hr_out want 4-byte alignment), so one case per group runs with every such pointer one element off the grid
and must give the same bits.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as MG
import sr_mi355x as S
from sr_mi355x import _lib, api, metrics, synth
from sr_mi355x import metrics_device as D
from sr_mi355x import register as G
import test_gpu_parity as P
import test_gpu_ssim as TS

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
EB = {"f32": 4, "f64": 8}
PRECS = ("f32", "f64")
CUDA = "cuda"
_HD = _lib._HD


TEST_IDS = []  # every parametrize id of this file, as pytest sees them (tests/test_memguard_host.py compares them with include/srx.h)


def ids(names):
    names = list(names)
    TEST_IDS.extend(names)
    return names


def lib():
    return _lib.load()


def fn(name, prec):
    return getattr(lib(), f"{name}_{prec}")


def hd(a):
    """host float64 array -> (array kept alive, pointer)"""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_HD)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def out(shape, dtype, skip=0):
    return MG.Guarded.tensor(shape, dtype, CUDA, skip=skip)


def put(x, skip=0):
    """an input tensor inside a guarded allocation, `skip` elements off the 256-byte grid; ends where the guard begins"""
    g = MG.Guarded.tensor(tuple(x.shape), x.dtype, CUDA, skip=skip)
    g.t.copy_(x)
    return g.t


def rnd(shape, prec, seed, integer=True):
    rng = np.random.default_rng(seed)
    a = np.rint(rng.uniform(0, 255, shape))
    if not integer:
        a = a * 0.75 + 0.3
    return torch.from_numpy(a).to(CUDA, DT[prec])


def contract(call, outs, need=None, inputs=(), poisons=MG.POISONS, short=True):
    """call(ws_ptr, ws_bytes) -> status under MG.run_poisoned with a guarded workspace of exactly `need` bytes; then the same call with
    need - 1 bytes: SRX_E_WORKSPACE, every guard intact, nothing stored (outputs and arena still hold their poison)."""
    ws = MG.Guarded(need, CUDA) if need is not None else None
    wsl = [ws] if ws is not None else []
    res = MG.run_poisoned(lambda: call(ctypes.c_void_p(ws.ptr) if ws is not None else None, ctypes.c_size_t(need or 0)), outs, wsl, inputs, poisons)
    if ws is not None and short:
        refused(call, outs, need)
    return res


def refused(call, outs, need):
    assert need > 0
    ws = MG.Guarded(need - 1, CUDA)
    for g in outs:
        g.fill(MG.POISON_GARBAGE)
    st = call(ctypes.c_void_p(ws.ptr), ctypes.c_size_t(need - 1))
    torch.cuda.synchronize()
    assert st == _lib.E_WORKSPACE, f"ws_bytes = need - 1 = {need - 1}: status {st}"
    ws.check("short workspace")
    assert ws.untouched(), "a refused call stored into its (short) workspace"
    for i, g in enumerate(outs):
        g.check(f"short workspace: output {i}")
        assert g.untouched(), f"a refused call stored into output {i}"
    # ... and a workspace off the 256-byte grid is refused on the host as well
    wm = MG.Guarded(need + 64, CUDA)
    st = call(ctypes.c_void_p(wm.ptr + 64), ctypes.c_size_t(need))
    torch.cuda.synchronize()
    assert st == _lib.E_WORKSPACE, f"misaligned workspace: status {st}"
    assert wm.untouched() and all(g.untouched() for g in outs)
    wm.check("misaligned workspace")


def same(a, b, what=""):
    assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"{what}: the guarded result differs from the wrapper's"


# =====================================================================================================================================
# primitives
# =====================================================================================================================================
_ASYM = synth.asymmetric_psf()
PRIM_SHAPES = {
    # name: (B, (H, W), PSF, (sy, sx), factor, also with element-aligned pointers)
    "B1_37x50_k7x7": (1, (37, 50), _ASYM, (0.37, -1.21), 2, True),                    # H, W odd against f = 2 on one axis
    "B3_5x1_k5x3": (3, (5, 1), _ASYM[1:6, 2:5] / _ASYM[1:6, 2:5].sum(), (7.5, -3.25), 2, False),  # |shift| larger than the image
    "B1_300x577_k15x15": (1, (300, 577), np.outer(np.hanning(17)[1:-1], np.hanning(17)[1:-1]) / np.outer(np.hanning(17)[1:-1], np.hanning(17)[1:-1]).sum(),
                          (0.9445, -0.8677), 4, False),                                # lines longer than a prefilter chunk; 577 = 4 * 144 + 1
}
PRIM_FUNCS = ("srx_blur", "srx_shift_cubic", "srx_zoom_cubic", "srx_forward", "srx_backproject")
PRIM_CASES = [(f, pr, s) for f in PRIM_FUNCS for pr in PRECS for s in PRIM_SHAPES]


def _prim(func, prec, shape, skip):
    B, (H, W), psf, (sy, sx), f, _ = PRIM_SHAPES[shape]
    dt, eb, L = DT[prec], EB[prec], lib()
    k, kp = hd(psf)
    kh, kw = k.shape
    x = put(rnd((B, H, W), prec, 11), skip)
    st = api._stream()
    if func == "srx_blur":
        o = out((B, H, W), dt, skip)
        return (lambda wp, wn: fn(func, prec)(p(x), B, H, W, kp, kh, kw, p(o.t), st)), [o], None, [x], lambda: [S.blur_batched(x, k, precision=prec)]
    if func == "srx_shift_cubic":
        o = out((B, H, W), dt, skip)
        return ((lambda wp, wn: fn(func, prec)(p(x), B, H, W, sy, sx, p(o.t), wp, wn, st)), [o], L.srx_shift_workspace_bytes(eb, B, H, W), [x],
                lambda: [S.shift_batched(x, (sy, sx), precision=prec)])
    if func == "srx_zoom_cubic":
        o = out((B, H * 2, W * 2), dt, skip)
        return ((lambda wp, wn: fn(func, prec)(p(x), B, H, W, 2, p(o.t), wp, wn, st)), [o], L.srx_zoom_workspace_bytes(eb, B, H, W, 2), [x],
                lambda: [S.zoom_batched(x, 2, precision=prec)])
    oh, ow = -(-H // f), -(-W // f)
    if func == "srx_forward":
        o = out((B, oh, ow), dt, skip)
        return ((lambda wp, wn: fn(func, prec)(p(x), B, H, W, kp, kh, kw, sy / f, sx / f, f, p(o.t), wp, wn, st)), [o],
                L.srx_forward_workspace_bytes(eb, B, H, W), [x], lambda: [S.forward_model_batched(x, k, (sy / f, sx / f), f, precision=prec)])
    e = put(rnd((B, oh, ow), prec, 12) - 128, skip)  # back_project: err [B, ceil(H / f), ceil(W / f)] -> [B, H, W], H, W no multiples of f
    o = out((B, H, W), dt, skip)
    return ((lambda wp, wn: fn(func, prec)(p(e), B, oh, ow, kp, kh, kw, sy / f, sx / f, f, H, W, p(o.t), wp, wn, st)), [o],
            L.srx_backproject_workspace_bytes(eb, B, H, W), [e], lambda: [S.back_project_batched(e, k, (sy / f, sx / f), f, (H, W), precision=prec)])


@pytest.mark.parametrize("func,prec,shape", PRIM_CASES, ids=ids(f"{f}_{pr}-{s}" for f, pr, s in PRIM_CASES))
def test_primitives(func, prec, shape):
    first = None
    for skip in (0, 1) if PRIM_SHAPES[shape][5] else (0,):
        call, outs, need, inputs, wrapper = _prim(func, prec, shape, skip)
        res = contract(call, outs, need, inputs)
        for a, b in zip(res, wrapper()):
            same(a, b, func)
        if first is not None:  # element-aligned pointers: the same bits
            assert all(torch.equal(a, b) for a, b in zip(first, res))
        first = res


# =====================================================================================================================================
# shift-and-add
# =====================================================================================================================================
SAA_CASES = {
    # name: (precisions, B, factor, shifts, (h, w), flags, path, also element-aligned)
    "two_pass_x3": (PRECS, 2, 3, synth.phase_shifts(3), (41, 57), 0, "mosaic", True),
    "one_pass_x3": (PRECS, 2, 3, synth.phase_shifts(3), (41, 57), S.FLAG_DIAG_SAA_ONE_PASS, "mosaic", False),
    "two_pass_x4_ragged": (PRECS, 1, 4, synth.phase_shifts(4)[:7], (100, 30), 0, "mosaic", False),
    "two_pass_below_a_tile": (PRECS, 1, 2, synth.phase_shifts(2), (9, 11), 0, "mosaic", False),
    "per_frame": (PRECS, 2, 2, synth.MEASURED_4, (45, 61), S.FLAG_PER_FRAME, "fused", True),
    "per_frame_of_a_common_fraction": (PRECS, 1, 4, synth.phase_shifts(4), (33, 20), S.FLAG_PER_FRAME, "fused", False),
    "below_the_fused_minimum": (PRECS, 2, 2, [(0.25, 0.0), (-0.25, 0.0)], (5, 1), 0, "composed", True),
    "chunked_2100x16": (("f32",), 2100, 4, synth.phase_shifts(4), (8, 8), 0, "mosaic", False),  # B * N > 32768: chunks of 2048 items inside the library
}
SAA_IDS = [(pr, c) for c, v in SAA_CASES.items() for pr in v[0]]


@pytest.mark.parametrize("prec,case", SAA_IDS, ids=ids(f"srx_saa_{pr}-{c}" for pr, c in SAA_IDS))
def test_shift_and_add(prec, case):
    _, B, f, shifts, (h, w), flags, path, misaligned = SAA_CASES[case]
    N, eb = len(shifts), EB[prec]
    sh, shp = hd(shifts)
    need = lib().srx_saa_workspace_bytes(eb, B, N, h, w, f)
    first = None
    for skip in (0, 1) if misaligned else (0,):
        x = put(rnd((B, N, h, w), prec, 21, integer=(case != "per_frame")), skip)
        o = out((B, h * f, w * f), DT[prec], skip)
        call = lambda wp, wn: fn("srx_saa", prec)(p(x), B, N, h, w, shp, f, p(o.t), wp, wn, api._stream(), flags)  # noqa: E731
        res = contract(call, [o], need, [x])
        assert S.last_path() == path
        same(res[0], S.shift_and_add_batched(x, sh, f, precision=prec, flags=flags), case)
        assert S.last_path() == path
        assert first is None or torch.equal(first, res[0])
        first = res[0]


# =====================================================================================================================================
# srx_ibp: one case per value of srx_last_path(), in every precision that path admits
# =====================================================================================================================================
_PSF = {"gauss": synth.gaussian_psf(), "asym": _ASYM, "full7": synth.full_support_psf(), "asym5": _ASYM[1:6, 1:6] / _ASYM[1:6, 1:6].sum()}
_FLAGS = {0: 0, "wide": S.FLAG_DIAG_WIDE_WINDOWS, "two": S.FLAG_DIAG_TWO_LAUNCH, "tiles": S.FLAG_TILES, "col": S.FLAG_DIAG_COLUMN_TILES,
          "composed": S.FLAG_COMPOSED, "per_frame_tiles": S.FLAG_TILES | S.FLAG_PER_FRAME, "7x7": S.FLAG_DIAG_NO_SEPARABLE}


def _ibp_case(name, path, prec, f, shifts, hw, psf="gauss", flags=0, integer=True, B=2, n_iter=2, misaligned=False):
    return dict(name=name, path=path, prec=prec, f=f, shifts=list(shifts), hw=hw, psf=psf, flags=_FLAGS[flags], integer=integer, B=B, n_iter=n_iter,
                misaligned=misaligned)


def _from(table, key, path, prec, **kw):
    """a configuration of the parity tests' tables: FUSED_CFGS (f, shifts, psf, hw, ...), DTILE_CFGS / ATILE_CFGS (f, shifts, hw, flags, ...)"""
    c = table[key]
    if table is P.FUSED_CFGS:
        return _ibp_case(f"{key}", path, prec, c[0], c[1], c[3], psf=c[2], **kw)
    if table is P.BTILE_CFGS:
        return _ibp_case(f"{key}", path, prec, 2, c[0], c[1], psf="gauss" if c[2] == "gauss7x7" else ("full7" if c[2] == "full7" else c[2]),
                         flags="7x7" if c[2] == "gauss7x7" else 0, **kw)
    if table is P.PATCH_CFGS or table is P.PATCH_CFGS_7X7:
        return _ibp_case(f"{key}", path, prec, c[0], c[1], (256 // c[0], 256 // c[0]), psf=c[3] if len(c) > 3 else "gauss", integer=c[2], n_iter=3, **kw)
    flags = c[3]
    integer = c[4] if len(c) > 4 else kw.pop("integer", True)
    return _ibp_case(f"{key}", path, prec, c[0], c[1], c[2], psf=c[5] if len(c) > 5 else "gauss", flags=flags, integer=integer, **kw)


IBP_CASES = [
    # patch (float32): byte mosaic + 0/1 masks, float mosaic, a count plane, the 7 x 7 form (5 x 5 core and full support)
    _from(P.PATCH_CFGS, "x4_grid", "patch", "f32", misaligned=True),
    _from(P.PATCH_CFGS, "x4_grid_float", "patch", "f32"),
    _from(P.PATCH_CFGS, "x4_dup", "patch", "f32"),
    _from(P.PATCH_CFGS, "x2_half_row", "patch", "f32"),
    _from(P.PATCH_CFGS_7X7, "x4_grid_asym", "patch", "f32"),
    _from(P.PATCH_CFGS_7X7, "x4_lattice_float_full7", "patch", "f32"),
    # stile (float64, rank-1 PSF): byte and float64 mosaic, a count plane
    _from(P.PATCH_CFGS, "x4_grid", "stile", "f64", misaligned=True),
    _from(P.PATCH_CFGS, "x4_grid_float", "stile", "f64"),
    _from(P.PATCH_CFGS, "x4_dup", "stile", "f64"),
    # ctile: float64 by default, float32 on request
    _from(P.FUSED_CFGS, "f2_nom5", "ctile", "f64", B=1),
    _from(P.FUSED_CFGS, "f2_nom4_big", "ctile", "f64", B=1, integer=False),
    _from(P.FUSED_CFGS, "f2_nom5", "ctile", "f32", B=1, flags="col", misaligned=True),
    _from(P.FUSED_CFGS, "f3_int_odd", "ctile", "f32", B=2, flags="col", integer=False),
    # ztile (float32): rank-1 and both 7 x 7 forms, packed and float operand planes, ragged last tiles, an odd HR height
    _from(P.FUSED_CFGS, "f2_nom5", "ztile", "f32", B=1, misaligned=True),
    _from(P.FUSED_CFGS, "f2_nom4_big", "ztile", "f32", B=1, integer=False),
    _from(P.FUSED_CFGS, "f3_int_odd", "ztile", "f32"),
    _from(P.FUSED_CFGS, "f3_ph9", "ztile", "f32", B=1),
    _from(P.FUSED_CFGS, "f2_nom5_full7", "ztile", "f32", B=1, integer=False),
    # dtile (float32): narrow and wide windows, byte and float mosaic, a count plane, the 7 x 7 form
    _from(P.DTILE_CFGS, "x4_ph16_narrow", "dtile", "f32", B=1, misaligned=True),
    _from(P.DTILE_CFGS, "x4_ph16_wide", "dtile", "f32", B=2),
    _from(P.DTILE_CFGS, "x4_ph16_float", "dtile", "f32", B=1),
    _from(P.DTILE_CFGS, "x2_ph4_w240", "dtile", "f32", B=1),
    _from(P.DTILE_CFGS, "x4_lattice", "dtile", "f32", B=1),
    _from(P.DTILE_CFGS, "x2_ph4_asym", "dtile", "f32", B=1),
    # atile (float32, rank-1 PSF)
    _from(P.ATILE_CFGS, "x4_ph16_small", "atile", "f32", misaligned=True),
    _from(P.ATILE_CFGS, "x2_ph4_ragged", "atile", "f32", B=1, integer=False),
    _from(P.ATILE_CFGS, "x4_lattice", "atile", "f32", B=1),
    _from(P.ATILE_CFGS, "x3_frac", "atile", "f32", B=1),
    _from(P.ATILE_CFGS, "x4_ph16_forced", "atile", "f32", B=1),
    # mosaic (the tile kernels; both precisions): integer and fractional HR shifts, rank-1 and 7 x 7, a frame below one tile
    _from(P.FUSED_CFGS, "f4_nom4", "mosaic", "f32", misaligned=True),
    _from(P.FUSED_CFGS, "f4_nom4", "mosaic", "f64"),
    _from(P.FUSED_CFGS, "f2_mixed", "mosaic", "f32", B=1, flags="tiles", integer=False),
    _from(P.FUSED_CFGS, "f2_multi", "mosaic", "f64", B=1, flags="tiles", integer=False, misaligned=True),
    _from(P.FUSED_CFGS, "f4_frac", "mosaic", "f32", B=1),
    _from(P.FUSED_CFGS, "f4_frac", "mosaic", "f64", B=1),
    _from(P.FUSED_CFGS, "f2_nom5", "mosaic", "f32", B=1, flags="tiles"),
    _ibp_case("x2_16x16", "mosaic", "f64", 2, synth.phase_shifts(2), (16, 16)),
    # btile (float32, x2, per-frame shifts)
    _from(P.BTILE_CFGS, "smallest", "btile", "f32"),
    _from(P.BTILE_CFGS, "tiny", "btile", "f32", misaligned=True),
    _from(P.BTILE_CFGS, "five_wide", "btile", "f32", B=1),
    _from(P.BTILE_CFGS, "tiny_asym", "btile", "f32"),
    _from(P.BTILE_CFGS, "smallest_asym5", "btile", "f32", B=1),
    _from(P.BTILE_CFGS, "meas4_gauss_as_7x7", "btile", "f32", B=1),
    # fused (per-frame tile kernels; both precisions)
    _from(P.FUSED_CFGS, "f3_k5", "fused", "f32", misaligned=True),
    _from(P.FUSED_CFGS, "f3_k5", "fused", "f64"),
    _from(P.FUSED_CFGS, "f2_meas", "fused", "f32", B=1, flags="per_frame_tiles"),
    _from(P.FUSED_CFGS, "f2_meas", "fused", "f64", B=1, integer=False),
    # composed (both precisions): on request, and the shapes below the fused minimum
    _from(P.FUSED_CFGS, "f3_k5", "composed", "f32", flags="composed"),
    _from(P.FUSED_CFGS, "f3_k5", "composed", "f64", flags="composed", misaligned=True),
    _ibp_case("3x7", "composed", "f32", 2, synth.NOMINAL_4, (3, 7), psf="asym", misaligned=True),   # 6 x 14 HR: below the fused paths' 8 x 8
    _ibp_case("5x1", "composed", "f64", 2, [(0.25, 0.0), (-0.25, 0.0)], (5, 1), psf="asym"),
    _ibp_case("2x9_N1", "composed", "f32", 3, [(0.1, 0.2)], (2, 9), psf="asym5", B=3),   # 6 x 27 HR
]
# Shapes beside "one case per path", held to the same contract.  A list of its own: tools/ws_sweep.py prints a block of
# tests/golden/workspace_bytes.txt per entry of IBP_CASES, and that file stays as the parent of the carve functions printed it.
IBP_MORE_CASES = [
    # dtile: 272 x 208 HR -- two windows on each axis (three near-band tables), ragged last 32 x 32 tiles of the operand planes on both axes
    _from(P.DTILE_CFGS, "x4_ph16_2x2win", "dtile", "f32", B=2),
]


def _ibp_id(c):
    fl = f"-flags0x{c['flags']:x}" if c["flags"] else ""
    return f"srx_ibp_{c['prec']}-{c['path']}-{c['name']}{fl}"


@pytest.mark.parametrize("c", IBP_CASES + IBP_MORE_CASES, ids=ids(_ibp_id(c) for c in IBP_CASES + IBP_MORE_CASES))
def test_ibp(c):
    prec, f, (h, w), B, n_iter, flags = c["prec"], c["f"], c["hw"], c["B"], c["n_iter"], c["flags"]
    dt, eb, L = DT[prec], EB[prec], lib()
    N, H, W = len(c["shifts"]), h * f, w * f
    sh, shp = hd(c["shifts"])
    k, kp = hd(_PSF[c["psf"]])
    kh, kw = k.shape
    need = L.srx_ibp_workspace_bytes_for(eb, B, N, h, w, H, W, f, shp, kp, kh, kw, flags)
    bound = L.srx_ibp_workspace_bytes(eb, B, N, h, w, H, W, f, flags)
    assert 0 < need <= bound
    ibp = fn("srx_ibp", prec)
    first = None
    for skip in (0, 1) if c["misaligned"] else (0,):
        lr = put(rnd((B, N, h, w), prec, 31, c["integer"]), skip)
        init = put(rnd((B, H, W), prec, 32, integer=False), skip)
        # out of place, the MSE trace guarded, the arena of exactly srx_ibp_workspace_bytes_for(); need - 1 is refused
        hr, errs = out((B, H, W), dt, skip), out((B, n_iter), torch.float64, skip)
        call = lambda wp, wn: ibp(p(lr), B, N, h, w, shp, kp, kh, kw, p(init), H, W, f, n_iter, 0.5, p(hr.t), p(errs.t), wp, wn, api._stream(), flags)  # noqa: E731
        res = contract(call, [hr, errs], need, [lr, init])
        assert S.last_path() == c["path"]
        w_hr, w_errs = S.ibp_batched(lr, sh, k, init, f, n_iter, 0.5, precision=prec, flags=flags)
        assert S.last_path() == c["path"]
        same(res[0], w_hr, "hr"), same(res[1], w_errs, "errors")
        # in place (hr_out == hr_init), no trace, the arena of the shape-only bound
        buf = out((B, H, W), dt, skip)
        buf.preset = init.clone()
        call2 = lambda wp, wn: ibp(p(lr), B, N, h, w, shp, kp, kh, kw, p(buf.t), H, W, f, n_iter, 0.5, p(buf.t), None, wp, wn, api._stream(), flags)  # noqa: E731
        res2 = contract(call2, [buf], bound, [lr], short=False)
        assert S.last_path() == c["path"]
        assert torch.equal(res2[0], res[0]), "in place / without the trace: a different state"
        if first is not None:  # element-aligned pointers: the same bits
            assert torch.equal(first[0], res[0]) and torch.equal(first[1], res[1])
        first = res


# =====================================================================================================================================
# plans
# =====================================================================================================================================
PLAN_CASES = {
    # name: (prec, f, shifts, (h, w), psf, B, plan path)
    "ztile_hoisted": ("f32", 2, synth.NOMINAL_5, (131, 200), "gauss", 1, "ztile"),
    "ztile_hoisted_batch_7x7": ("f32", 3, P.FUSED_CFGS["f3_ph9"][1], (50, 66), "asym", 2, "ztile"),
    "call_per_run_ctile": ("f64", 2, synth.NOMINAL_5, (131, 200), "gauss", 1, "call per run"),
    "call_per_run_atile": ("f32", 4, synth.phase_shifts(4), (40, 50), "gauss", 2, "call per run"),
}


def _plan_id(name):
    pr = PLAN_CASES[name][0]
    return f"srx_ibp_plan_create_{pr}-srx_ibp_plan_run-srx_ibp_plan_get_rows_{pr}-srx_ibp_plan_set_rows_{pr}-{name}"


@pytest.mark.parametrize("name", list(PLAN_CASES), ids=ids(_plan_id(n) for n in PLAN_CASES))
def test_plan(name):
    prec, f, shifts, (h, w), psf, B, path = PLAN_CASES[name]
    dt, eb, L = DT[prec], EB[prec], lib()
    N, H, W = len(shifts), h * f, w * f
    sh, shp = hd(shifts)
    k, kp = hd(_PSF[psf])
    kh, kw = k.shape
    need = L.srx_ibp_plan_workspace_bytes(eb, B, N, h, w, H, W, f, 0)
    lo, hi = H // 3, H // 3 + 5
    create, get_rows, set_rows = fn("srx_ibp_plan_create", prec), fn("srx_ibp_plan_get_rows", prec), fn("srx_ibp_plan_set_rows", prec)
    first = None
    for skip in (0, 1):  # on the 256-byte grid, then every caller pointer (frames, state, rows in and out, traces) one element off it
        lr, init = put(rnd((B, N, h, w), prec, 41), skip), put(rnd((B, H, W), prec, 42, integer=False), skip)
        rows_in = put(rnd((B, hi - lo, W), prec, 43, integer=False), skip)
        e1, e2 = out((B, 2), torch.float64, skip), out((B, 1), torch.float64, skip)
        mid, last, full = out((B, hi - lo, W), dt, skip), out((B, 1, W), dt, skip), out((B, H, W), dt, skip)
        seen = {}

        def call(wp, wn):
            st, h_ = api._stream(), ctypes.c_void_p()
            rc = create(p(lr), B, N, h, w, shp, kp, kh, kw, p(init), H, W, f, 0.5, 0, H, wp, wn, st, 0, ctypes.byref(h_))
            if rc != _lib.OK:
                assert not h_
                return rc
            try:
                seen["path"] = L.srx_ibp_plan_path(h_).decode()
                for step in (lambda: L.srx_ibp_plan_run(h_, 2, p(e1.t), st), lambda: get_rows(h_, lo, hi, p(mid.t), st),
                             lambda: get_rows(h_, H - 1, H, p(last.t), st), lambda: set_rows(h_, lo, hi, p(rows_in), st),
                             lambda: L.srx_ibp_plan_run(h_, 1, p(e2.t), st), lambda: get_rows(h_, 0, H, p(full.t), st)):
                    rc = step()
                    if rc != _lib.OK:
                        return rc
                torch.cuda.synchronize()
                return _lib.OK
            finally:
                L.srx_ibp_plan_destroy(h_)

        res = contract(call, [e1, mid, last, e2, full], need, [lr, init, rows_in])
        assert seen["path"] == path
        pl = api.IbpPlan(lr, sh, k, init, f, 0.5, precision=prec)
        assert pl.path == path
        w1 = pl.run(2)
        wm, wl = pl.get_rows(lo, hi), pl.get_rows(H - 1, H)
        pl.set_rows(lo, hi, rows_in)
        w2 = pl.run(1)
        wf = pl.result()
        pl.close()
        for a, b, what in zip(res, (w1, wm, wl, w2, wf), ("errors of run 1", "interior rows", "last row", "errors of run 2", "state")):
            same(a, b, what)
        assert first is None or all(torch.equal(a, b) for a, b in zip(first, res)), "element-aligned pointers: different bits"
        first = res


# =====================================================================================================================================
# index maps and pointwise glue (bit-exact kernels; uint8 outputs poisoned with 0xA5 / 0x5A)
# =====================================================================================================================================
def _u8(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).to(CUDA)


def _index_map(func, prec, size, skip):
    """-> (call, outputs, inputs, poisons, wrapper)"""
    dt, st = DT[prec] if prec else None, api._stream()
    small = size == "1x1"
    if prec:
        S.set_precision(prec)  # (the single-image wrappers work in the process precision; test_index_maps restores it)
    if func == "srx_decimate":
        B, (H, W), f, py, px = (1, (1, 1), 2, 0, 0) if small else (2, (37, 51), 3, 1, 2)
        x, o = put(rnd((B, H, W), prec, 51), skip), out((B, -(-(H - py) // f), -(-(W - px) // f)), dt, skip)
        return (lambda: fn(func, prec)(p(x), B, H, W, f, py, px, p(o.t), st)), [o], [x], MG.POISONS, lambda: [torch.stack([S.decimate(x[i], f, py, px) for i in range(B)])]
    if func == "srx_zero_insert":
        B, (eh, ew), f, (H, W) = (1, (1, 1), 2, (1, 1)) if small else (2, (13, 17), 3, (37, 50))
        x, o = put(rnd((B, eh, ew), prec, 52), skip), out((B, H, W), dt, skip)
        return ((lambda: fn(func, prec)(p(x), B, eh, ew, f, H, W, p(o.t), st)), [o], [x], MG.POISONS,
                lambda: [torch.stack([S.zero_insert(x[i], f, (H, W)) for i in range(B)])])
    if func == "srx_mean_frames":
        B, R, n = (1, 1, 1) if small else (2, 3, 37 * 51)  # 1887: no multiple of 4, 64 or 256
        x, o = put(rnd((B, R, n), prec, 53, integer=False), skip), out((B, n), dt, skip)
        return (lambda: fn(func, prec)(p(x), B, R, ctypes.c_size_t(n), p(o.t), st)), [o], [x], MG.POISONS, lambda: [S.mean_frames_batched(x)]
    n = 1 if small else 1887
    if func == "srx_u8_to":
        x, o = put(_u8((n,), 54), skip), out((n,), dt, skip)
        return (lambda: fn(func, prec)(p(x), ctypes.c_size_t(n), p(o.t), st)), [o], [x], MG.POISONS, lambda: [S.u8_to_float(x, precision=prec)]
    if func == "srx_quantize_u8":
        x, o = put(rnd((n,), prec, 55, integer=False) * 1.2 - 20, skip), out((n,), torch.uint8, skip)
        return (lambda: fn(func, prec)(p(x), ctypes.c_size_t(n), p(o.t), st)), [o], [x], MG.INT_POISONS, lambda: [S.quantize_u8(x)]
    B, h, w = (1, 1, 1) if small else (2, 5, 7)
    x, o = put(_u8((B, 4, h, w), 56), skip), out((B, 2 * h, 2 * w), torch.uint8, skip)
    return (lambda: lib().srx_interleave4_u8(p(x), B, h, w, p(o.t), st)), [o], [x], MG.INT_POISONS, lambda: [S.interleave4(x)]


INDEX_CASES = [(f, pr, s) for f in ("srx_decimate", "srx_zero_insert", "srx_mean_frames", "srx_u8_to", "srx_quantize_u8") for pr in PRECS
               for s in ("odd", "1x1")] + [("srx_interleave4_u8", None, s) for s in ("odd", "1x1")]


@pytest.mark.parametrize("func,prec,size", INDEX_CASES, ids=ids((f"{f}_{pr}" if pr else f) + f"-{s}" for f, pr, s in INDEX_CASES))
def test_index_maps(func, prec, size):
    before = S.get_precision()
    try:
        first = None
        for skip in (0, 1):
            call, outs, inputs, poisons, wrapper = _index_map(func, prec, size, skip)
            res = MG.run_poisoned(call, outs, (), inputs, poisons)
            for a, b in zip(res, wrapper()):
                same(a, b, func)
            assert first is None or torch.equal(first[0], res[0])
            first = res
    finally:
        S.set_precision(before)


# =====================================================================================================================================
# metrics: the workspace of exactly srx_metrics_workspace_bytes at the call's own sizes
# =====================================================================================================================================
def _pair(shape, prec, B=None, seed=0):
    ps = [TS.pair(*shape, seed=seed + i) for i in range(B or 1)]
    a, b = np.stack([q[0] for q in ps]), np.stack([q[1] for q in ps])
    return (torch.from_numpy(a if B else a[0]).to(CUDA, DT[prec]), torch.from_numpy(b if B else b[0]).to(CUDA, DT[prec]))


METRIC_SHAPES = {f"{h}x{w}": (h, w) for h, w in TS.SHAPES}
PAIR_CASES = [(pr, s, b) for pr in PRECS for s in METRIC_SHAPES for b in (0, 3)]


@pytest.mark.parametrize("prec,shape,border", PAIR_CASES, ids=ids(f"srx_pair_moments_{pr}-{s}-border{b}" for pr, s, b in PAIR_CASES))
def test_pair_moments(prec, shape, border):
    B, (H, W) = 2, METRIC_SHAPES[shape]
    first = None
    for skip in (0, 1) if shape == "61x97" else (0,):
        a, b = (put(x, skip) for x in _pair((H, W), prec, B, seed=3))
        o = out((B, 7), torch.float64, skip)
        need = lib().srx_metrics_workspace_bytes(B, H, W, 1)
        res = contract(lambda wp, wn: fn("srx_pair_moments", prec)(p(a), p(b), B, H, W, border, p(o.t), wp, wn, api._stream()), [o], need, [a, b])
        assert np.array_equal(res[0].cpu().numpy(), D.pair_moments(a, b, border=border))
        assert first is None or torch.equal(first, res[0])
        first = res[0]


SSIM_CASES = {
    # name: (shape, B, radius, border, map, affine)
    "61x97_r3_border3_map": ("61x97", 2, 3, 3, True, False),
    "61x97_r1_mean_only": ("61x97", 1, 1, 0, False, False),
    "300x517_r7_map_affine": ("300x517", 2, 7, 0, True, True),
    "300x517_r5_border10_mean_only_affine": ("300x517", 1, 5, 10, False, True),
    "15x300_r7_map": ("15x300", 1, 7, 0, True, False),   # the window as tall as the image
    "15x300_r1_border2_map": ("15x300", 3, 1, 2, True, False),
}
SSIM_IDS = [(pr, c) for pr in PRECS for c in SSIM_CASES]


@pytest.mark.parametrize("prec,case", SSIM_IDS, ids=ids(f"srx_ssim_{pr}-{c}" for pr, c in SSIM_IDS))
def test_ssim(prec, case):
    shape, B, radius, border, want_map, want_affine = SSIM_CASES[case]
    H, W = METRIC_SHAPES[shape]
    h, w = H - 2 * border, W - 2 * border
    first = None
    for skip in (0, 1) if case == "61x97_r3_border3_map" else (0,):
        a, b = (put(x, skip) for x in _pair((H, W), prec, B, seed=5))
        rad, taps, dr = metrics.ssim_params((h, w), np.float64, 2 * radius + 1, 255.0, False, 1.5)
        assert rad == radius
        taps, tp = hd(taps)
        aff_h = np.array([[1.0, 0.9 + 0.05 * i, 4.0 - i] for i in range(B)]) if want_affine else None
        aff = put(torch.from_numpy(aff_h).to(CUDA), skip) if want_affine else None
        m, smap = out((B,), torch.float64, skip), out((B, h, w), DT[prec], skip) if want_map else None
        need = lib().srx_metrics_workspace_bytes(B, H, W, 1)
        call = lambda wp, wn: fn("srx_ssim", prec)(p(a), p(b), B, H, W, border, radius, tp, 1, dr, 0.01, 0.03, p(aff), p(m.t),  # noqa: E731
                                                   p(smap.t) if want_map else None, wp, wn, api._stream())
        res = contract(call, [m] + ([smap] if want_map else []), need, [a, b] + ([aff] if want_affine else []))
        wr = D._ssim(a, b, prec, False, np.float64, aff_h, win_size=2 * radius + 1, data_range=255.0, border=border, full=want_map)
        assert res[0].cpu().tolist() == (wr[0] if want_map else wr)
        if want_map:
            same(res[1], wr[1], "SSIM map")
        assert first is None or all(torch.equal(x, y) for x, y in zip(first, res))
        first = res


PROFILE_CASES = [(pr, n, win) for pr in PRECS for n, win in ((97, 20), (1, 4), (300, 16), (517, 33))]


def _local_contrast_ref(x, window):
    """metrics.local_contrast in the tensor's own precision: (max - min) / (max + min + 1e-9) of profile[i - w/2 : i + w/2], 0 within w/2
    of either end.  Maxima, one subtraction, two additions and one correctly rounded division: the same bits as the kernel's."""
    B, n = x.shape
    hw, res = window // 2, torch.zeros_like(x)
    if hw > 0 and n >= 2 * hw + 1:
        win = x.unfold(1, 2 * hw, 1)[:, :n - 2 * hw]  # window s = profile[s : s + 2 hw] belongs to i = s + hw, i < n - hw
        mx, mn = win.max(dim=2).values, win.min(dim=2).values
        res[:, hw:n - hw] = (mx - mn) / (mx + mn + torch.tensor(1e-9, dtype=x.dtype, device=x.device))
    return res


@pytest.mark.parametrize("prec,n,window", PROFILE_CASES, ids=ids(f"srx_local_contrast_{pr}-n{n}-window{w_}" for pr, n, w_ in PROFILE_CASES))
def test_local_contrast(prec, n, window):
    B = 3
    first = None
    for skip in (0, 1):
        x, o = put(rnd((B, n), prec, 61, integer=False), skip), out((B, n), DT[prec], skip)
        res = MG.run_poisoned(lambda: fn("srx_local_contrast", prec)(p(x), B, n, window, p(o.t), api._stream()), [o], (), [x])
        same(res[0], _local_contrast_ref(x, window), "local contrast")
        if prec == "f64":  # (the wrapper works in float64 only)
            assert np.array_equal(res[0].cpu().numpy(), D.local_contrast(x, window=window))
        assert first is None or torch.equal(first, res[0])
        first = res[0]


ROI_CASES = [(pr, s) for pr in PRECS for s in METRIC_SHAPES]


@pytest.mark.parametrize("prec,shape", ROI_CASES, ids=ids(f"srx_ring_sums_{pr}-srx_spot_moments_{pr}-{s}" for pr, s in ROI_CASES))
def test_ring_sums_and_spot_moments(prec, shape):
    H, W = METRIC_SHAPES[shape]
    first = None
    for skip in (0, 1) if shape == "61x97" else (0,):
        img = put(_pair((H, W), prec, seed=7)[0], skip)
        cy, cx = 0.5 * H - 0.25, 0.5 * W + 1.5
        nbin = int(min(cy, cx, H - cy, W - cx))
        rings = out((2 * nbin,), torch.float64, skip)
        need = lib().srx_metrics_workspace_bytes(1, H, W, nbin)
        r = contract(lambda wp, wn: fn("srx_ring_sums", prec)(p(img), H, W, cy, cx, nbin, p(rings.t), wp, wn, api._stream()), [rings], need, [img])
        o = r[0].cpu().numpy()
        radii, means = D.radial_average(img, (cy, cx), nbin)
        assert np.array_equal(np.divide(o[:nbin], o[nbin:], out=np.zeros(nbin), where=o[nbin:] > 0), means)
        spot = out((4,), torch.float64, skip)
        s = MG.run_poisoned(lambda: fn("srx_spot_moments", prec)(p(img), H, W, p(spot.t), api._stream()), [spot], (), [img])
        _, mass, sy, sx = s[0].cpu().numpy()
        assert (float(sy / mass), float(sx / mass)) == D.subpixel_centre(img)
        assert first is None or (torch.equal(first[0], r[0]) and torch.equal(first[1], s[0]))
        first = (r[0], s[0])


EDGE_IDS = list(METRIC_SHAPES)


def _edge_roi(H, W):
    """an 8-bit slanted edge (integer values: the float32 and float64 bins then add the same numbers), along the longer side"""
    r, c = np.mgrid[:H, :W].astype(np.float64)
    d = (c - 0.1 * r - 0.45 * W) if W <= 2 * H else (r - 0.02 * c - 0.3 * H)
    return np.round(40.0 + 170.0 / (1.0 + np.exp(-d / 1.2)))


def _edge_fit(mag, side="left"):
    """the host part of metrics_device.slanted_edge_esf between its device calls: the line through the edge pixels of one side"""
    rs, cs = np.where(mag > np.percentile(mag, 85))
    rows_are_x = bool((rs.max() - rs.min()) >= (cs.max() - cs.min()))
    u, v = (rs, cs) if rows_are_x else (cs, rs)
    m_c, b_c = np.polyfit(u, v, 1)
    edge_dist = (v - m_c * u - b_c) / np.sqrt(1 + m_c ** 2)
    sel = edge_dist < 0 if side == "left" else edge_dist > 0
    m, b = np.polyfit(u[sel], v[sel], 1)
    return float(m), float(b), float(np.sqrt(1 + m ** 2)), int(rows_are_x)


def _esf(o, lo, hi):
    """... and behind them: bin centres and the interpolated, oriented edge-spread function"""
    bins = np.arange(lo, hi + 0.25, 0.25)
    esf_x = 0.5 * (bins[:-1] + bins[1:])
    nbin = len(esf_x)
    tot, cnt = o[:nbin], o[nbin:]
    esf_y = np.full(nbin, np.nan)
    np.divide(tot, cnt, out=esf_y, where=cnt > 0)
    valid = ~np.isnan(esf_y)
    if valid.sum() > 2:
        esf_y = np.interp(esf_x, esf_x[valid], esf_y[valid])
    if esf_y[-1] < esf_y[0]:
        esf_x, esf_y = -esf_x[::-1], esf_y[::-1]
    return esf_x, esf_y


@pytest.mark.parametrize("shape", EDGE_IDS, ids=ids(f"srx_edge_magnitude_f64-srx_edge_dist_range-srx_edge_bins_f32-srx_edge_bins_f64-{s}" for s in EDGE_IDS))
def test_edge_metrics(shape):
    """The three device steps of metrics_device.slanted_edge_esf, guarded, with its host steps in between (_edge_fit, _esf): the edge-spread
    function that comes out is the wrapper's, bit for bit, so the range and the bins are tied to it; the float32 bins of an 8-bit ROI
    equal the float64 ones."""
    H, W = METRIC_SHAPES[shape]
    L, st = lib(), api._stream()
    first = None
    for skip in (0, 1) if shape == "61x97" else (0,):
        roi = put(torch.from_numpy(_edge_roi(H, W)).to(CUDA), skip)
        w_x, w_y, _ = D.slanted_edge_esf(roi)
        mag = out((H, W), torch.float64, skip)
        need = L.srx_metrics_workspace_bytes(1, H, W, 1)
        r_mag = contract(lambda wp, wn: L.srx_edge_magnitude_f64(p(roi), H, W, 1.5, p(mag.t), wp, wn, st), [mag], need, [roi])
        same(r_mag[0], D.edge_magnitude(roi), "edge magnitude")
        m, b, norm, rows_are_x = _edge_fit(r_mag[0].cpu().numpy())
        rng = out((2,), torch.float64, skip)
        r_rng = MG.run_poisoned(lambda: L.srx_edge_dist_range(H, W, m, b, norm, rows_are_x, p(rng.t), st), [rng])
        lo, hi = (float(v) for v in r_rng[0].cpu().numpy())
        nbin = len(np.arange(lo, hi + 0.25, 0.25)) - 1
        res = [r_mag[0], r_rng[0]]
        for prec in PRECS:
            x = put(roi.to(DT[prec]), skip)
            bins = out((2 * nbin,), torch.float64, skip)
            need = L.srx_metrics_workspace_bytes(1, H, W, nbin)
            res += contract(lambda wp, wn: fn("srx_edge_bins", prec)(p(x), H, W, m, b, norm, rows_are_x, lo, 0.25, nbin, p(bins.t), wp, wn, st), [bins], need, [x])
            g_x, g_y = _esf(res[-1].cpu().numpy(), lo, hi)
            assert np.array_equal(g_x, w_x) and np.array_equal(g_y, w_y), f"{prec}: the edge-spread function differs from slanted_edge_esf's"
        assert first is None or all(torch.equal(x, y) for x, y in zip(first, res))
        first = res


# =====================================================================================================================================
# registration
# =====================================================================================================================================
REG_CASES = {
    # name: (B, (H, W), search, border, score / status pointers)
    "search0_border0": (1, (48, 64), 0, 0, True),
    "search4_border2": (1, (48, 64), 4, 2, True),
    "search4_border0_no_score_no_status": (1, (48, 64), 4, 0, False),
    "smallest_16x16_crop": (1, (26, 26), 2, 1, True),   # 16 + 2 (border + search + 2)
    "B3_odd_shape": (3, (75, 131), 2, 3, True),
    "B3_no_score_no_status": (3, (75, 131), 1, 0, False),
}
REG_IDS = [(pr, c) for pr in PRECS for c in REG_CASES]


@pytest.mark.parametrize("prec,case", REG_IDS, ids=ids(f"srx_register_{pr}-{c}" for pr, c in REG_IDS))
def test_register(prec, case):
    B, (H, W), search, border, with_score = REG_CASES[case]
    N, n_iter, tol = 4, 4, 1e-4
    base = torch.from_numpy(synth.truth_image(H + 8, W + 8, seed=13)).to(CUDA, DT[prec])
    frames = torch.stack([torch.stack([base[4 + dy + b:4 + dy + b + H, 4 + dx:4 + dx + W] for dy, dx in ((0, 0), (1, 0), (0, -1), (-1, 1))]) for b in range(B)])
    frames = torch.round(0.6 * frames + 0.4 * torch.roll(frames, 1, dims=3))  # integer offsets plus half a pixel of blur along x
    need = lib().srx_register_workspace_bytes(EB[prec], B, N, H, W, search)
    assert need > 0
    first = None
    for skip in (0, 1) if case == "B3_odd_shape" else (0,):
        x = put(frames, skip)
        sh, sc, stt = out((B, N, 2), torch.float64, skip), out((B, N), torch.float64, skip), out((B, N), torch.int32, skip)
        outs = [sh, sc, stt] if with_score else [sh]
        call = lambda wp, wn: fn("srx_register", prec)(p(x), B, N, H, W, 0, None, search, border, n_iter, tol, p(sh.t),  # noqa: E731
                                                       p(sc.t) if with_score else None, p(stt.t) if with_score else None, wp, wn, api._stream())
        res = contract(call, outs, need, [x])
        d, s, st = G.estimate_shifts(x, search=search, border=border, n_iter=n_iter, tol=tol, precision=prec, full=True)
        assert np.array_equal(res[0].cpu().numpy(), d.reshape(B, N, 2))
        if with_score:
            assert np.array_equal(res[1].cpu().numpy(), s.reshape(B, N)) and np.array_equal(res[2].cpu().numpy(), st.reshape(B, N))
        assert first is None or all(torch.equal(a, b) for a, b in zip(first, res))
        first = res


# =====================================================================================================================================
# the test files that declare memory-contract cases of their own through ids() above
REGISTERING_FILES = ("test_gpu_items", "test_gpu_register_u8", "test_gpu_psf", "test_gpu_u8lr")


def all_case_ids():
    """every memory-contract test id: those the parametrize calls above registered and those of REGISTERING_FILES, which register theirs on
    import (imported here, not at the top: they import this module)"""
    import importlib
    for name in REGISTERING_FILES:
        importlib.import_module(name)
    return list(TEST_IDS)
