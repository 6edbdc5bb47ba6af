"""Registration on the camera's bytes (srx_register_u8_*, estimate_shifts on uint8 input, session.register_shifts with keep_u8 loaders).

The contract is bit identity: srx_register_u8_T returns the shifts, scores and status codes of srx_register_T on the frames converted with
srx_u8_to_T.  The shapes are the smallest at which each part of the byte kernels can go wrong (odd sizes and a stack that starts off the
4-byte grid, partial column chunks, several chunks per coarse block, one offset and 81 offsets, the 16 x 16 crop, windows that leave the
frame, samples of 0 and 255 only).  One case also goes through the independent oracle of tests/register_oracle.py with the tolerances of
tests/test_gpu_register.py; the workspace rule, the error table and the memory contract (tests/memguard.py) are held at the C ABI."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import memguard as MG
import register_oracle as R
import test_gpu_memory_contract as MC
from oracle import sr_oracle as O
from sr_mi355x import _lib, api, session, synth
from sr_mi355x import register as G

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
EB = {"f32": 4, "f64": 8}
PRECS = ("f32", "f64")


def sensor_u8(truth, shifts, f=2, seed=1):
    """the existing tests' recipe: the oracle's forward model, sigma = 1 noise, rint, clip, uint8"""
    psf = synth.gaussian_psf()
    lr = np.stack([O.forward_model(truth, psf, s, f) for s in shifts])
    lr = lr + np.random.default_rng(seed).normal(0.0, 1.0, lr.shape)
    return np.clip(np.rint(lr), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_frames(name):
    """-> (frames uint8 [B, N, H, W] (read-only), keyword arguments of the call); computed once and shared"""
    m4, n5 = np.asarray(synth.MEASURED_4), np.asarray(synth.NOMINAL_5)
    if name == "256":
        fr, kw = sensor_u8(synth.truth_image(256, 256), m4), dict(init=m4)
    elif name == "odd":  # H W and W odd; crop 138 x 265: two refinement strips, five coarse column chunks, the last 9 wide
        fr, kw = sensor_u8(synth.truth_image(300, 554, seed=7), n5)[:, :150, :277], dict(init=n5, ref=2, search=1, border=3, n_iter=6)
    elif name in ("search0", "search4"):  # one offset and 256 groups; 81 offsets, three groups, thirteen idle lanes
        fr, kw = sensor_u8(synth.truth_image(128, 192, seed=3), m4), dict(init=m4, search=int(name[-1]))
    elif name == "crop16_s2":
        fr, kw = sensor_u8(synth.truth_image(52, 52, seed=9), m4), dict(init=m4, search=2, border=1)
    elif name == "crop16_s4":
        fr, kw = sensor_u8(synth.truth_image(56, 56, seed=9), m4), dict(init=m4, search=4, border=0)
    elif name == "two_chunks":  # crop 292 x 1092: 18 column chunks, crow = 32 (two 16-row chunks per coarse block)
        fr, kw = sensor_u8(synth.truth_image(600, 2200, seed=5), m4[:3]), dict(init=m4[:3], search=2, border=0)
    elif name == "outside":  # margin 4, starts of 7 and 6 pixels: the coarse window and the clamped tap columns leave the frame
        base = sensor_u8(synth.truth_image(192, 256, seed=6), [(0.0, 0.0)])[0]
        fr = np.stack([base, np.roll(base, (7, -6), axis=(0, 1)), np.roll(base, (-7, 5), axis=(0, 1))])
        kw = dict(init=np.array([[0.0, 0.0], [7.0, -6.0], [-7.0, 5.0]]), search=2, border=0)
    elif name == "extreme":  # samples 0 and 255 only (the largest products), and one flat frame of 255
        base = np.where(sensor_u8(synth.truth_image(256, 256, seed=8), [(0.0, 0.0)])[0] >= 128, 255, 0).astype(np.uint8)
        fr = np.stack([base, np.roll(base, (1, -1), axis=(0, 1)), np.full_like(base, 255), np.roll(base, (-2, 1), axis=(0, 1))])
        kw = dict()
    elif name == "batch":
        nom = np.asarray(synth.NOMINAL_4)
        tr = nom + np.random.default_rng(5).uniform(-0.2, 0.2, nom.shape)
        fr = np.stack([sensor_u8(synth.truth_image(192, 224, seed=s), tr + 0.05 * s, seed=s) for s in range(3)])
        kw = dict(init=nom)
    else:
        raise KeyError(name)
    fr = np.ascontiguousarray(fr if fr.ndim == 4 else fr[None])
    fr.setflags(write=False)
    return fr, kw


def on_device(fr, offset=0):
    """the stack on the device; offset: a view starting that many bytes into a flat buffer"""
    flat = torch.empty(offset + fr.size, dtype=torch.uint8, device="cuda")
    x = flat[offset:].view(fr.shape)
    x.copy_(torch.from_numpy(fr.copy()))
    return x


def call_abi(name, prec, x, shifts, score, status, ws_ptr, ws_bytes, ref=0, init=None, search=2, border=8, n_iter=10, tol=1e-4, N=None, null_frames=False):
    B, n, H, W = x.shape
    hinit = None if init is None else np.ascontiguousarray(init, dtype=np.float64)
    return getattr(_lib.load(), f"{name}_{prec}")(
        None if null_frames else api._p(x), B, n if N is None else N, H, W, ref, None if hinit is None else hinit.ctypes.data_as(_lib._HD), search,
        border, n_iter, tol, None if shifts is None else api._p(shifts), None if score is None else api._p(score),
        None if status is None else api._p(status), ws_ptr, ctypes.c_size_t(ws_bytes), api._stream())


def run(kind, prec, x, **kw):
    """kind 'u8': srx_register_u8_T on the bytes; 'float': srx_register_T on srx_u8_to_T of them -> (shifts, score, status) on the host"""
    lib = _lib.load()
    B, N, H, W = x.shape
    if kind == "float":
        src = x.clone()
        xf = torch.empty(x.shape, dtype=DT[prec], device="cuda")
        _lib.check(getattr(lib, f"srx_u8_to_{prec}")(api._p(src), ctypes.c_size_t(src.numel()), api._p(xf), api._stream()), "srx_u8_to")
        x = xf
    shifts = torch.full((B, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    score = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((B, N), -1, dtype=torch.int32, device="cuda")
    need = lib.srx_register_workspace_bytes(EB[prec], B, N, H, W, kw.get("search", 2))
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = call_abi("srx_register_u8" if kind == "u8" else "srx_register", prec, x, shifts, score, status, api._p(ws), need, **kw)
    assert rc == _lib.OK, (kind, rc)
    torch.cuda.synchronize()
    return shifts.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


# ---- 1. the same bits as the float call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["256", "odd", "search0", "search4", "crop16_s2", "crop16_s4", "two_chunks", "outside", "extreme"])
def test_same_bits_as_the_float_call(name, prec):
    fr, kw = case_frames(name)
    x = on_device(fr, offset=1 if name == "odd" else 0)
    assert name != "odd" or x.data_ptr() % 4 == 1
    got, want = run("u8", prec, x, **kw), run("float", prec, x, **kw)
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]), (got[1], want[1])
    assert np.array_equal(got[2], want[2]), (got[2], want[2])
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    ref = kw.get("ref", 0)
    assert np.array_equal(got[0][0, ref], [0.0, 0.0]) and got[1][0, ref] == 1.0 and got[2][0, ref] == 0
    if name == "extreme":
        assert got[2][0, 2] == 1  # the flat frame: singular, the coarse shift kept (finite: checked above)
    if name == "outside":  # the rolled frames are found where init says they are
        assert np.abs(got[0][0] - kw["init"]).max() < 0.5
    if name == "two_chunks":  # (margin 4) 18 column chunks, and more 16-row chunks than the 15 block rows a frame of 18 columns gets
        assert -(-(fr.shape[3] - 8) // 64) == 18 and fr.shape[2] - 8 > 16 * 15


@pytest.mark.parametrize("prec", PRECS)
def test_batch_equals_items_runs_and_the_float_batch(prec):
    fr, kw = case_frames("batch")
    x = on_device(fr)
    a, b = run("u8", prec, x, **kw), run("u8", prec, x, **kw)
    assert same(a, b)
    assert same(a, run("float", prec, x, **kw))
    for i in range(fr.shape[0]):
        one = run("u8", prec, on_device(fr[i:i + 1]), **kw)
        assert same([v[i:i + 1] for v in a], one), i


# ---- 2. against the independent oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_against_the_oracle(prec):
    fr, kw = case_frames("256")
    d_o, s_o, st_o, _ = R.register_item(fr[0].astype(np.float64), **kw)
    d, s, st = (v[0] for v in run("u8", prec, on_device(fr), **kw))
    assert np.array_equal(st, st_o), (st, st_o)
    assert np.abs(d - d_o).max() <= (1e-8 if prec == "f64" else 1e-3), (d, d_o)
    assert np.abs(s - s_o).max() <= (1e-10 if prec == "f64" else 1e-4), (s, s_o)


# ---- 3. workspace and errors at the C ABI ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_workspace_rule(prec):
    fr, _ = case_frames("search0")
    x = on_device(fr)
    B, N, H, W = x.shape
    shifts = torch.empty((B, N, 2), dtype=torch.float64, device="cuda")
    for search in (0, 2, 4):
        need = _lib.load().srx_register_workspace_bytes(EB[prec], B, N, H, W, search)
        raw = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
        off = (-raw.data_ptr()) % 256
        base = raw.data_ptr() + off
        for ptr, nb, want in ((base, need, _lib.OK), (base, need - 1, _lib.E_WORKSPACE), (base + 4, need, _lib.E_WORKSPACE),
                              (base + 128, need, _lib.E_WORKSPACE)):
            rc = call_abi("srx_register_u8", prec, x, shifts, None, None, ctypes.c_void_p(ptr), nb, search=search, n_iter=3)
            assert rc == want, (search, ptr - base, nb, rc)
    torch.cuda.synchronize()
    assert np.all(np.isfinite(shifts.cpu().numpy()))


@pytest.mark.parametrize("prec", PRECS)
def test_error_table_is_the_float_call_s(prec):
    lib = _lib.load()
    x8 = torch.zeros((1, 4, 40, 40), dtype=torch.uint8, device="cuda")
    xf = torch.zeros((1, 4, 40, 40), dtype=DT[prec], device="cuda")
    out = torch.empty((1, 4, 2), dtype=torch.float64, device="cuda")
    n = lib.srx_register_workspace_bytes(EB[prec], 1, 4, 40, 40, 4)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")

    def call(name, x, **kw):
        a = dict(shifts=out, ref=0, search=2, border=2, n_iter=3, tol=1e-4, N=None, null_frames=False)
        a.update(kw)
        return call_abi(name, prec, x, a.pop("shifts"), None, None, api._p(ws), n, **a)

    table = [(dict(), _lib.OK), (dict(null_frames=True), _lib.E_INVALID), (dict(shifts=None), _lib.E_INVALID), (dict(ref=4), _lib.E_INVALID),
             (dict(ref=-1), _lib.E_INVALID), (dict(search=-1), _lib.E_INVALID), (dict(search=5), _lib.E_INVALID), (dict(n_iter=-1), _lib.E_INVALID),
             (dict(tol=float("nan")), _lib.E_INVALID), (dict(border=-1), _lib.E_INVALID), (dict(border=8), _lib.OK),  # crop 40 - 2 (8 + 2 + 2) = 16
             (dict(border=9), _lib.E_UNSUPPORTED),  # a crop of 15
             (dict(N=33), _lib.E_UNSUPPORTED)]
    for kw, want in table:
        got8, gotf = call("srx_register_u8", x8, **kw), call("srx_register", xf, **kw)
        assert got8 == want and gotf == want, (kw, got8, gotf, want)
    torch.cuda.synchronize()


# ---- 4. the memory contract -----------------------------------------------------------------------------------------------------------
# (the ids are registered with tests/test_gpu_memory_contract.py's list, which tests/test_memguard_host.py compares with include/srx.h)
@pytest.mark.parametrize("case", MC.ids(f"srx_register_u8_{pr}-odd_byte_150x277" for pr in PRECS))
def test_memory_contract(case):
    prec = case.split("-")[0][-3:]
    fr, kw = case_frames("odd")
    B, N, H, W = fr.shape
    xg = MG.Guarded.tensor(fr.shape, torch.uint8, "cuda", skip=1)  # one byte off the 256-byte grid, ending where the guard begins
    xg.t.copy_(torch.from_numpy(fr.copy()))
    sh = MG.Guarded.tensor((B, N, 2), torch.float64, "cuda")
    sc = MG.Guarded.tensor((B, N), torch.float64, "cuda")
    st = MG.Guarded.tensor((B, N), torch.int32, "cuda")
    need = _lib.load().srx_register_workspace_bytes(EB[prec], B, N, H, W, kw["search"])
    # every poison of the module in turn, guards around outputs and workspace, the input compared with its clone; then need - 1 bytes: refused
    res = MC.contract(lambda wp, wn: call_abi("srx_register_u8", prec, xg.t, sh.t, sc.t, st.t, wp, wn.value, **kw), [sh, sc, st], need, [xg.t])
    xg.check("frames")
    assert same([r.cpu().numpy() for r in res], run("float", prec, xg.t, **kw))


# ---- 5. Python and the session driver -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS)
def test_estimate_shifts_takes_bytes_in_every_form(prec):
    fr, kw = case_frames("256")
    fr = fr[0]
    want = G.estimate_shifts(fr.astype(np.float64), precision=prec, full=True, **kw)
    for frames in (fr.copy(), torch.from_numpy(fr.copy()).cuda(), [a.copy() for a in fr], [torch.from_numpy(a.copy()).cuda() for a in fr]):
        got = G.estimate_shifts(frames, precision=prec, full=True, **kw)
        assert same(got, want), type(frames)
    b = G.estimate_shifts(np.stack([fr, fr]), precision=prec, full=True, **kw)  # [B, N, H, W] bytes
    assert b[0].shape == (2, 4, 2) and same([v[0] for v in b], want) and same([v[1] for v in b], want)


def test_session_keep_u8_writes_the_same_files(tmp_path, monkeypatch):
    from PIL import Image
    table = np.asarray(session.CORNER_SHIFTS, dtype=np.float64)
    sess = tmp_path / "data" / "barcodes"
    sess.mkdir(parents=True)
    for rep in range(2):
        true = table + np.random.default_rng(10 + rep).uniform(-0.15, 0.15, table.shape)
        for c, fr in enumerate(sensor_u8(synth.truth_image(256, 288, seed=5 + rep), true, seed=rep)):
            Image.fromarray(fr).save(sess / f"corner{c}_rep{rep:02d}.png")
    seen = []
    real = G.estimate_shifts

    def spy(frames, *a, **kw):
        seen.append((frames.dtype, tuple(frames.shape)))
        return real(frames, *a, **kw)

    monkeypatch.setattr(G, "estimate_shifts", spy)
    psf = synth.gaussian_psf()
    out = {}
    for keep in (True, False):
        dirs = session.process_session(str(sess), psf, str(tmp_path / f"u8_{keep}"), kind="mono_barcodes", n_iter=3, verbose=False, register=True,
                                       keep_u8=keep)
        assert [os.path.basename(d) for d in dirs] == ["rep0", "rep1"]
        out[keep] = [{n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))} for d in dirs]
    assert seen == [(torch.uint8, (2, 4, 128, 144)), (torch.float64, (2, 4, 128, 144))]
    assert out[True] == out[False]
    for files in out[True]:
        assert "registration.json" in files and "SAA.png" in files
        assert json.loads(files["registration.json"])["status"] == [0] * 4
