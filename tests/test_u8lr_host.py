"""srx_saa_u8lr_* / srx_ibp_u8lr_* / srx_decimate_u8 without a GPU: the names, the argument checks the library makes before any HIP call (fake
pointers are never dereferenced), the workspace rules of include/srx.h, and the memory-contract ids tests/test_memguard_host.py asks for."""
import ctypes

import numpy as np
import pytest

import test_abi
import test_gpu_u8lr  # noqa: F401  (declares the memory-contract cases of the uint8 entry points on import, see the last test)
from sr_mi355x import _lib, synth

FAKE = ctypes.c_void_p(4096)
NEW = ("srx_saa_u8lr_workspace_bytes", "srx_saa_u8lr_f32", "srx_saa_u8lr_f64", "srx_ibp_u8lr_workspace_bytes", "srx_ibp_u8lr_workspace_bytes_for",
       "srx_ibp_u8lr_f32", "srx_ibp_u8lr_f64", "srx_decimate_u8")
CHUNK = 32768  # items of one launch (larger batches go through in chunks)


def lib():
    return _lib.load()


def hd(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_lib._HD)


def align_up(n):
    return -(-n // 256) * 256


def test_header_ctypes_table_and_library_agree():
    hdr, L = test_abi.header_symbols(), lib()
    for name in NEW:
        assert name in hdr and name in _lib.symbols() and hasattr(L, name), name
    assert "srx_saa_u8lr_{T}" in _lib._TYPED and "srx_ibp_u8lr_{T}" in _lib._TYPED
    assert _lib._TYPED["srx_saa_u8lr_{T}"] == _lib._TYPED["srx_saa_{T}"] and _lib._TYPED["srx_ibp_u8lr_{T}"] == _lib._TYPED["srx_ibp_{T}"]
    for plain in ("srx_saa_u8lr_workspace_bytes", "srx_ibp_u8lr_workspace_bytes", "srx_ibp_u8lr_workspace_bytes_for", "srx_decimate_u8"):
        assert plain in _lib._PLAIN
    import sr_mi355x
    for name in ("shift_and_add_u8_batched", "ibp_u8_batched", "decimate_u8", "extract_red_u8"):
        assert name in sr_mi355x.__all__


SH, SHP = hd(synth.phase_shifts(2))
K, KP = hd(synth.gaussian_psf())


def _ibp_args(ws=FAKE, wsb=1 << 30):
    # lr, B, N, h, w, shifts, kernel, kh, kw, hr_init, H, W, f, n_iter, step, hr_out, errors, ws, ws_bytes, stream, flags
    return [FAKE, 2, 4, 16, 16, SHP, KP, 7, 7, FAKE, 32, 32, 2, 2, 0.5, FAKE, None, ws, wsb, None, 0]


def _saa_args(ws=FAKE, wsb=1 << 30):
    # lr, B, N, h, w, shifts, f, out, ws, ws_bytes, stream, flags
    return [FAKE, 2, 4, 16, 16, SHP, 2, FAKE, ws, wsb, None, 0]


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_arguments_are_refused_without_gpu(prec):
    L = lib()
    ibp, saa = getattr(L, f"srx_ibp_u8lr_{prec}"), getattr(L, f"srx_saa_u8lr_{prec}")
    for i, bad in ((0, None), (5, None), (6, None), (9, None), (15, None), (1, 0), (1, -1), (2, 0), (3, 0), (4, -2), (7, 0), (8, 0), (10, 0), (11, -1),
                   (12, 0), (13, -1)):
        a = _ibp_args()
        a[i] = bad
        assert ibp(*a) == _lib.E_INVALID, (i, bad)
    for i, bad in ((0, None), (5, None), (7, None), (1, 0), (2, 0), (3, -1), (4, 0), (6, 0)):
        a = _saa_args()
        a[i] = bad
        assert saa(*a) == _lib.E_INVALID, (i, bad)
    ok = [FAKE, 1, 8, 8, 2, 0, 0, FAKE, None]  # in, B, H, W, f, py, px, out, stream
    for i, bad in ((0, None), (7, None), (1, 0), (4, 0), (5, -1), (6, -1), (5, 8), (6, 8)):
        a = list(ok)
        a[i] = bad
        assert L.srx_decimate_u8(*a) == _lib.E_INVALID, (i, bad)
    assert L.srx_decimate_u8(FAKE, 65536, 8, 8, 2, 0, 0, FAKE, None) == _lib.E_UNSUPPORTED


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_unsupported_sizes_are_refused_without_gpu(prec):
    """The float call's limits: N <= 32, kh kw <= 225, and planes below 2 GiB COUNTED IN T (the state and the tables are T)."""
    L = lib()
    ibp, saa = getattr(L, f"srx_ibp_u8lr_{prec}"), getattr(L, f"srx_saa_u8lr_{prec}")
    sh33, p33 = hd(np.zeros((33, 2)))
    a = _ibp_args()
    a[2], a[5] = 33, p33
    assert ibp(*a) == _lib.E_UNSUPPORTED
    a = _saa_args()
    a[2], a[5] = 33, p33
    assert saa(*a) == _lib.E_UNSUPPORTED
    k16, p16 = hd(np.full((16, 15), 1.0 / 240))
    a = _ibp_args()
    a[6], a[7], a[8] = p16, 16, 15
    assert ibp(*a) == _lib.E_UNSUPPORTED
    side = 1 << 15  # 32768 x 32768 HR: 4 GiB in float32
    a = _ibp_args()
    a[3], a[4], a[10], a[11] = side // 2, side // 2, side, side
    assert ibp(*a) == _lib.E_UNSUPPORTED
    a = _saa_args()
    a[3], a[4] = side // 2, side // 2
    assert saa(*a) == _lib.E_UNSUPPORTED
    # invalid wins over unsupported
    a = _ibp_args()
    a[2], a[5], a[0] = 33, p33, None
    assert ibp(*a) == _lib.E_INVALID


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_workspace_is_checked_without_gpu(prec):
    """Too short, null or off the 256-byte grid: SRX_E_WORKSPACE on the host, before anything is queued -- on a route that stages the frames
    as on one that does not."""
    L, eb = lib(), {"f32": 4, "f64": 8}[prec]
    ibp, saa = getattr(L, f"srx_ibp_u8lr_{prec}"), getattr(L, f"srx_saa_u8lr_{prec}")
    for shifts in (synth.phase_shifts(2), synth.MEASURED_4):
        _, shp = hd(shifts)
        need = L.srx_ibp_u8lr_workspace_bytes_for(eb, 2, 4, 16, 16, 32, 32, 2, shp, KP, 7, 7, 0)
        for ws, wsb in ((FAKE, need - 1), (None, need), (ctypes.c_void_p(4096 + 64), need)):
            a = _ibp_args(ws, wsb)
            a[5] = shp
            assert ibp(*a) == _lib.E_WORKSPACE
        need = L.srx_saa_u8lr_workspace_bytes(eb, 2, 4, 16, 16, 2)
        for ws, wsb in ((FAKE, need - 1), (None, need), (ctypes.c_void_p(4096 + 64), need)):
            a = _saa_args(ws, wsb)
            a[5] = shp
            assert saa(*a) == _lib.E_WORKSPACE


MOSAIC_FAMILY = {"patch", "stile", "ctile", "ztile", "dtile", "atile", "mosaic"}


def test_workspace_relations():
    """srx_ibp_u8lr_workspace_bytes_for = the float query on a mosaic-family route (nothing is staged: the kernels read the bytes), the float
    query + one chunk's frames in T elsewhere; the shape-only bound covers both.  A reduced form of tests/test_abi.py's sweep."""
    L = lib()
    psfs = [synth.gaussian_psf(), synth.asymmetric_psf(), synth.full_support_psf()]
    seen = set()
    for f, shift_sets in ((2, (synth.NOMINAL_4, synth.NOMINAL_5, synth.MEASURED_4, synth.phase_shifts(2))),
                          (3, (synth.phase_shifts(3),)), (4, (synth.phase_shifts(4), synth.NOMINAL_4))):
        for shifts in shift_sets:
            _, shp = hd(shifts)
            N = len(shifts)
            for H in (32, 132, 256, 320):
                for W in (64, 208, 256, 272):
                    if H % f or W % f:
                        continue
                    h, w = H // f, W // f
                    for psf in psfs:
                        _, kp = hd(psf)
                        for eb in (4, 8):
                            path = L.srx_ibp_path_for(eb, N, h, w, H, W, f, shp, kp, 7, 7, 0).decode()
                            seen.add(path)
                            for B in (1, 3, 130):
                                bound = L.srx_ibp_u8lr_workspace_bytes(eb, B, N, h, w, H, W, f, 0)
                                need = L.srx_ibp_u8lr_workspace_bytes_for(eb, B, N, h, w, H, W, f, shp, kp, 7, 7, 0)
                                fneed = L.srx_ibp_workspace_bytes_for(eb, B, N, h, w, H, W, f, shp, kp, 7, 7, 0)
                                what = (f, N, H, W, eb, B, path)
                                assert 0 < need <= bound, what
                                if path in MOSAIC_FAMILY:
                                    assert need == fneed, what
                                else:
                                    assert path in ("btile", "fused", "composed") and need == fneed + align_up(min(B, CHUNK) * N * h * w * eb), what
                                sneed = L.srx_saa_u8lr_workspace_bytes(eb, B, N, h, w, f)
                                assert sneed == L.srx_saa_workspace_bytes(eb, B, N, h, w, f) + align_up(B * N * h * w * eb), what
    assert {"patch", "stile", "btile", "fused", "mosaic"} <= seen  # the sweep meets both kinds of route
    # the batch beyond one launch: one chunk is staged, not the batch
    _, shp = hd(synth.MEASURED_4)
    a = L.srx_ibp_u8lr_workspace_bytes_for(4, 40000, 4, 8, 8, 16, 16, 2, shp, KP, 7, 7, 0)
    assert a == L.srx_ibp_workspace_bytes_for(4, 40000, 4, 8, 8, 16, 16, 2, shp, KP, 7, 7, 0) + align_up(CHUNK * 4 * 8 * 8 * 4)
    assert L.srx_saa_u8lr_workspace_bytes(4, 2100, 16, 8, 8, 4) == L.srx_saa_workspace_bytes(4, 2100, 16, 8, 8, 4) + align_up(2048 * 16 * 8 * 8 * 4)
    # without the tables the _for query is the bound
    assert L.srx_ibp_u8lr_workspace_bytes_for(4, 3, 4, 16, 16, 32, 32, 2, None, None, 7, 7, 0) == L.srx_ibp_u8lr_workspace_bytes(4, 3, 4, 16, 16, 32, 32, 2, 0)


def test_wrappers_check_the_dtype_before_the_device(monkeypatch):
    from sr_mi355x import api

    def no_device(*a, **k):
        raise AssertionError("the wrapper touched the device before checking its arguments")

    monkeypatch.setattr(api, "_device", no_device)
    for bad in (np.zeros((1, 4, 8, 8), np.float32), np.zeros((1, 4, 8, 8), np.int8), np.zeros((1, 4, 8, 8), bool)):
        with pytest.raises(TypeError):
            api.shift_and_add_u8_batched(bad, synth.NOMINAL_4, 2)
        with pytest.raises(TypeError):
            api.ibp_u8_batched(bad, synth.NOMINAL_4, synth.gaussian_psf(), np.zeros((1, 16, 16)), 2, 1)
    with pytest.raises(ValueError):
        api.shift_and_add_u8_batched(np.zeros((4, 8, 8), np.uint8), synth.NOMINAL_4, 2)   # [B, N, h, w] is asked for
    with pytest.raises(TypeError):
        api.decimate_u8(np.zeros((8, 8), np.float64), 2)


def test_memory_contract_cases_are_declared():
    """tests/test_memguard_host.py asks every device-output entry point of include/srx.h for a memory-contract case; those of the uint8
    entry points live in tests/test_gpu_u8lr.py and are registered in the same list."""
    import test_gpu_memory_contract as T
    import test_memguard_host as H
    ids = T.all_case_ids()
    assert set(test_gpu_u8lr.CONTRACT) <= set(ids)
    parsed = H.device_output_functions()
    for name in ("srx_saa_u8lr_f32", "srx_saa_u8lr_f64", "srx_ibp_u8lr_f32", "srx_ibp_u8lr_f64", "srx_decimate_u8"):
        assert name in parsed, f"{name}: include/srx.h declares no device output pointer for it"
        assert any(name in i.split("-") for i in ids), name
    # the ids follow the documented forms and every route has one in every precision it admits
    assert "srx_decimate_u8-37x50" in ids and "srx_saa_u8lr_f64-two_pass_x3" in ids and "srx_ibp_u8lr_f32-patch-x4_grid" in ids
    have = {tuple(i.split("-")[:2]) for i in ids if i.startswith("srx_ibp_u8lr_")}
    assert have == {(f"srx_ibp_u8lr_{c['prec']}", c["path"]) for c in T.IBP_CASES}
