"""srx_mean_u8's argument checks (include/srx.h): every refusal is decided on the host before any HIP call, so none of this needs a
GPU -- the pointers are never dereferenced."""
import ctypes

import pytest

from sr_mi355x import _lib

FAKE = ctypes.c_void_p(4096)
OK_ARGS = dict(inp=FAKE, B=1, R=2, H=4, W=6, f=2, py=0, px=0, eb=4, out=FAKE)


def call(**kw):
    a = dict(OK_ARGS, **kw)
    return _lib.load().srx_mean_u8(a["inp"], a["B"], a["R"], a["H"], a["W"], a["f"], a["py"], a["px"], a["eb"], a["out"], None)


INVALID = {
    "null_in": dict(inp=None), "null_out": dict(out=None),
    "B0": dict(B=0), "B_neg": dict(B=-1), "R0": dict(R=0), "R_neg": dict(R=-3), "H0": dict(H=0), "H_neg": dict(H=-4), "W0": dict(W=0), "W_neg": dict(W=-6),
    "f0": dict(f=0), "f_neg": dict(f=-2),
    "py_neg": dict(py=-1), "py_H": dict(py=4), "px_neg": dict(px=-1), "px_W": dict(px=6),
    "eb0": dict(eb=0), "eb1": dict(eb=1), "eb2": dict(eb=2), "eb16": dict(eb=16),
}
UNSUPPORTED = {
    "R65536": dict(R=65536),
    "B65536": dict(B=65536),
    "item_2GiB": dict(R=2, H=1 << 15, W=1 << 15),        # R H W = 2^31 exactly
    "item_2GiB_by_R": dict(R=32768, H=256, W=256),
    "frame_over_int": dict(R=1, H=1 << 16, W=1 << 16),   # H W alone does not fit an int
}


@pytest.mark.parametrize("case", list(INVALID))
def test_invalid_arguments(case):
    assert call(**INVALID[case]) == _lib.E_INVALID


@pytest.mark.parametrize("case", list(UNSUPPORTED))
def test_unsupported_arguments(case):
    assert call(**UNSUPPORTED[case]) == _lib.E_UNSUPPORTED


def test_invalid_wins_over_unsupported():
    assert call(R=65536, f=0) == _lib.E_INVALID


def test_the_largest_R_passes_the_host_checks():
    """R = 65535 (255 * 65535 < 2^24: the float32 sum is still exact) with a one-sample frame is no refusal: the call goes on to launch.
    Without a device that is SRX_E_HIP on the fake pointers.  With one the launch would run on them, so there the buffers are real (the
    result at this R is checked in tests/test_gpu_mean_u8.py)."""
    import torch
    inp, out, keep = FAKE, FAKE, None
    if torch.cuda.is_available():
        keep = (torch.zeros(65535, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
        inp, out = ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr())
    for eb in (4, 8):
        assert call(inp=inp, out=out, R=65535, H=1, W=1, f=1, eb=eb) not in (_lib.E_INVALID, _lib.E_UNSUPPORTED)
    if keep is not None:
        torch.cuda.synchronize()


def test_symbol_is_in_the_ctypes_table():
    assert "srx_mean_u8" in _lib.symbols()
