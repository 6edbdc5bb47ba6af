"""One shift table per item (srx_saa_items_*, srx_ibp_items_*): what the host decides, checked without a GPU -- the workspace queries are
host arithmetic, and a refused call returns before anything is queued (the device pointers below are placeholders nobody follows)."""
import ctypes

import numpy as np
import pytest

from sr_mi355x import _lib, api, synth

EB = {"f32": 4, "f64": 8}
LARGE = [(2.5, 0.0), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)]  # |f s| > 4 HR px: no fused form ("composed")
FAKE = ctypes.c_void_p(1 << 20)  # a device pointer the refused calls never reach


def lib():
    return _lib.load()


def hd(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_lib._HD)


def random_tables(rng, B, N):
    """B tables of N frames: nominal phases, measured-like fractions, a table beyond the fused reach, and runs of equal tables"""
    out = []
    while len(out) < B:
        kind = rng.integers(0, 4)
        nominal = np.asarray([(0.5 * rng.choice((-1, 1)), 0.5 * rng.choice((-1, 1))) for _ in range(N)])
        if kind == 0:
            t = nominal
        elif kind == 1:
            t = nominal + rng.uniform(-0.05, 0.05, (N, 2))
        elif kind == 2:
            t = rng.uniform(-1.9, 1.9, (N, 2))
        else:
            t = nominal.copy()
            t[0] = (2.5, 0.0)
        out += [t] * int(rng.integers(1, 3))
    return np.stack(out[:B])


def test_shape_only_bound_covers_every_table():
    rng = np.random.default_rng(5)
    L = lib()
    k, kp = hd(synth.gaussian_psf())
    k2, kp2 = hd(synth.asymmetric_psf())
    n = 0
    for prec in ("f32", "f64"):
        for f in (2, 3, 4):
            for (h, w) in ((16, 16), (24, 32), (64, 80), (33, 47), (200, 130)):
                for B, N in ((1, 4), (3, 4), (5, 2), (8, 9), (40000, 4)):
                    if B > 100 and (h, w) != (16, 16):
                        continue
                    sh, shp = hd(random_tables(rng, B, N))
                    for kk, kkp in ((k, kp), (k2, kp2)):
                        for flags in (0, _lib.FLAG_PER_FRAME, _lib.FLAG_COMPOSED, _lib.FLAG_TILES):
                            bound = L.srx_ibp_items_workspace_bytes(EB[prec], B, N, h, w, h * f, w * f, f, flags)
                            exact = L.srx_ibp_items_workspace_bytes_for(EB[prec], B, N, h, w, h * f, w * f, f, shp, kkp, kk.shape[0], kk.shape[1], flags)
                            assert 0 < exact <= bound, (prec, f, h, w, B, N, flags, exact, bound)
                            n += 1
    assert n > 500


def test_all_tables_equal_needs_what_the_shared_call_needs():
    L = lib()
    k, kp = hd(synth.gaussian_psf())
    for table in (synth.NOMINAL_4, synth.MEASURED_4, LARGE):
        one, onep = hd(table)
        sh, shp = hd(np.stack([one] * 3))
        a = L.srx_ibp_items_workspace_bytes_for(4, 3, 4, 64, 80, 128, 160, 2, shp, kp, 7, 7, 0)
        b = L.srx_ibp_workspace_bytes_for(4, 3, 4, 64, 80, 128, 160, 2, onep, kp, 7, 7, 0)
        assert a == b


def _ibp(name, B, N, sh, lr=FAKE, hr_init=FAKE, hr=FAKE, k=None, flags=0, ws=FAKE, wsb=1 << 30, h=64, w=80, f=2):
    kk, kp = hd(synth.gaussian_psf())
    return getattr(lib(), name)(lr, B, N, h, w, sh, kp if k is None else k, 7, 7, hr_init, h * f, w * f, f, 3, 0.5, hr, None, ws, wsb, None, flags)


def _saa(name, B, N, sh, lr=FAKE, out=FAKE, h=64, w=80, f=2, flags=0):
    return getattr(lib(), name)(lr, B, N, h, w, sh, f, out, FAKE, 1 << 30, None, flags)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_invalid_arguments_give_the_shared_calls_statuses(prec):
    sh, shp = hd(np.stack([synth.MEASURED_4] * 2))
    big, bigp = hd(np.zeros((2, _lib_max_frames() + 1, 2)))
    none_hd = ctypes.cast(None, _lib._HD)
    cases = [dict(lr=None), dict(hr_init=None), dict(hr=None), dict(sh=none_hd), dict(k=none_hd), dict(B=0), dict(B=-3),
             dict(N=_lib_max_frames() + 1, sh=bigp)]
    for c in cases:
        kw = dict(B=2, N=4, sh=shp)
        kw.update(c)
        got, want = _ibp(f"srx_ibp_items_{prec}", **kw), _ibp(f"srx_ibp_{prec}", **kw)
        assert got == want and got in (_lib.E_INVALID, _lib.E_UNSUPPORTED), (c, got, want)
    assert _ibp(f"srx_ibp_items_{prec}", 2, _lib_max_frames() + 1, bigp) == _lib.E_UNSUPPORTED
    # the four places that check an ibp call -- the call, its per-item form, a plan and srx_ibp_path_for ("none" stands for a refusal
    # there) -- answer one bad argument, and N = 33, alike: an invalid argument before a limit
    k, kp = hd(synth.gaussian_psf())
    for c, want in [(dict(sh=none_hd), _lib.E_INVALID), (dict(k=none_hd), _lib.E_INVALID), (dict(h=0), _lib.E_INVALID), (dict(f=0), _lib.E_INVALID),
                    (dict(N=33, sh=bigp), _lib.E_UNSUPPORTED), (dict(N=33, sh=bigp, h=0), _lib.E_INVALID)]:
        a = dict(B=2, N=4, sh=shp, k=kp, h=64, w=80, f=2)
        a.update(c)
        plan = ctypes.c_void_p()
        got = [_ibp(f"srx_ibp_{prec}", **a), _ibp(f"srx_ibp_items_{prec}", **a),
               getattr(lib(), f"srx_ibp_plan_create_{prec}")(FAKE, a["B"], a["N"], a["h"], a["w"], a["sh"], a["k"], 7, 7, FAKE, a["h"] * a["f"], a["w"] * a["f"],
                                                            a["f"], 0.5, 0, a["h"] * a["f"], FAKE, 1 << 30, None, 0, ctypes.byref(plan))]
        assert got == [want] * 3 and not plan.value, (c, got, want)
        assert lib().srx_ibp_path_for(EB[prec], a["N"], a["h"], a["w"], a["h"] * a["f"], a["w"] * a["f"], a["f"], a["sh"], a["k"], 7, 7, 0) == b"none", c
    for c in [dict(lr=None), dict(out=None), dict(sh=none_hd), dict(B=0), dict(N=_lib_max_frames() + 1, sh=bigp)]:
        kw = dict(B=2, N=4, sh=shp)
        kw.update(c)
        got, want = _saa(f"srx_saa_items_{prec}", **kw), _saa(f"srx_saa_{prec}", **kw)
        assert got == want and got in (_lib.E_INVALID, _lib.E_UNSUPPORTED), (c, got, want)


def _lib_max_frames():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(re.search(r"#define SRX_MAX_FRAMES (\d+)", open(os.path.join(root, "include", "srx.h")).read()).group(1))


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_flag_fused_is_refused_when_one_item_cannot_fuse(prec):
    sh, shp = hd(np.stack([synth.MEASURED_4, synth.MEASURED_4, LARGE]))
    assert _ibp(f"srx_ibp_items_{prec}", 3, 4, shp, flags=_lib.FLAG_FUSED) == _lib.E_UNSUPPORTED
    assert _saa(f"srx_saa_items_{prec}", 3, 4, shp, flags=_lib.FLAG_FUSED) == _lib.E_UNSUPPORTED
    # ... and a short or misaligned workspace, before anything is queued
    ok, okp = hd(np.stack([synth.MEASURED_4] * 3))
    need = lib().srx_ibp_items_workspace_bytes_for(EB[prec], 3, 4, 64, 80, 128, 160, 2, okp, hd(synth.gaussian_psf())[1], 7, 7, 0)
    assert _ibp(f"srx_ibp_items_{prec}", 3, 4, okp, wsb=need - 1) == _lib.E_WORKSPACE
    assert _ibp(f"srx_ibp_items_{prec}", 3, 4, okp, ws=ctypes.c_void_p((1 << 20) + 64), wsb=need) == _lib.E_WORKSPACE


def test_api_rejects_other_table_shapes():
    B, N = 3, 4
    lr = np.zeros((B, N, 8, 8))
    hr = np.zeros((B, 16, 16))
    for bad in (np.zeros((B + 1, N, 2)), np.zeros((N, 3)), np.zeros((N * 2,)), np.zeros((B, N, 3))):
        with pytest.raises(ValueError):
            api.shift_and_add_batched(lr, bad, 2)
        with pytest.raises(ValueError):
            api.ibp_batched(lr, bad, synth.gaussian_psf(), hr, 2, 1)
        with pytest.raises(ValueError):
            api.shift_and_add_u8_batched(lr.astype(np.uint8), bad, 2)
        with pytest.raises(ValueError):
            api.ibp_u8_batched(lr.astype(np.uint8), bad, synth.gaussian_psf(), hr, 2, 1)
