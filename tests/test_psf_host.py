"""srx_psf_estimate_* without a GPU: the workspace query, the argument checks the library makes before any HIP call (null / fake
pointers are never dereferenced) and the wrapper's own argument errors, which are raised before any device work."""
import ctypes

import numpy as np
import pytest

import test_gpu_psf  # noqa: F401  (declares the memory-contract cases of srx_psf_estimate_* on import, see the last test)
from sr_mi355x import _lib

FAKE = ctypes.c_void_p(4096)
REF = (30, 1536, 2048, 3)  # the reference's calibration stack: 30 pinhole frames of 1536 x 2048, halfwidth 3


def lib():
    return _lib.load()


def entry_points():
    L = lib()
    return [(1, L.srx_psf_estimate_u8), (4, L.srx_psf_estimate_f32), (8, L.srx_psf_estimate_f64)]


def test_workspace_query():
    q = lib().srx_psf_estimate_workspace_bytes
    assert q(1, *REF) > 0 and q(1, *REF) % 256 == 0
    sizes = [q(1, n, 1536, 2048, 3) for n in (1, 2, 30, 31, 90)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]   # monotone in N
    assert q(1, *REF) <= q(4, *REF) <= q(8, *REF)
    for hw in (0, 8, -1):
        assert q(1, 30, 1536, 2048, hw) == 0
    for hw in range(1, 8):
        assert q(4, 30, 1536, 2048, hw) > 0
    # arguments no call accepts
    assert q(2, *REF) == 0 and q(0, *REF) == 0
    assert q(1, 0, 1536, 2048, 3) == 0 and q(1, 30, 0, 2048, 3) == 0 and q(1, 30, 1536, -1, 3) == 0
    assert q(1, 65536, 64, 64, 3) == 0 and q(1, 65535, 64, 64, 3) > 0
    assert q(1, 1, 1 << 15, 1 << 16, 3) == 0 and q(4, 1, 23200, 23200, 3) == 0


def test_invalid_arguments_are_refused_without_gpu():
    for eb, fn in entry_points():
        ok = (FAKE, 4, 64, 64, 3, FAKE, None, FAKE, 1 << 20, None)
        for i, bad in ((0, None), (5, None), (1, 0), (1, -1), (2, 0), (3, 0), (3, -5), (4, 0), (4, 8), (4, -1)):
            args = list(ok)
            args[i] = bad
            assert fn(*args) == _lib.E_INVALID, (eb, i, bad)


def test_unsupported_sizes_are_refused_without_gpu():
    """One frame of 2 GiB or more (32-bit indices inside a frame) and N > 65535 are SRX_E_UNSUPPORTED before any HIP call."""
    L = lib()
    assert L.srx_psf_estimate_u8(FAKE, 1, 1 << 15, 1 << 16, 3, FAKE, None, FAKE, 1 << 20, None) == _lib.E_UNSUPPORTED    # 2 GiB exactly
    assert L.srx_psf_estimate_f32(FAKE, 1, 23200, 23200, 3, FAKE, None, FAKE, 1 << 20, None) == _lib.E_UNSUPPORTED       # 2.15 GB
    assert L.srx_psf_estimate_f64(FAKE, 1, 1 << 14, 1 << 14, 3, FAKE, None, FAKE, 1 << 20, None) == _lib.E_UNSUPPORTED   # 2 GiB exactly
    for eb, fn in entry_points():
        assert fn(FAKE, 65536, 64, 64, 3, FAKE, None, FAKE, 1 << 20, None) == _lib.E_UNSUPPORTED, eb
    # invalid wins over unsupported, as everywhere in the library
    assert L.srx_psf_estimate_u8(FAKE, 65536, 64, 64, 0, FAKE, None, FAKE, 1 << 20, None) == _lib.E_INVALID


def test_workspace_is_checked_without_gpu():
    """Too short, null or off the 256-byte grid: SRX_E_WORKSPACE on the host, before anything is queued."""
    for eb, fn in entry_points():
        need = lib().srx_psf_estimate_workspace_bytes(eb, 4, 64, 64, 3)
        assert fn(FAKE, 4, 64, 64, 3, FAKE, None, FAKE, need - 1, None) == _lib.E_WORKSPACE
        assert fn(FAKE, 4, 64, 64, 3, FAKE, None, None, need, None) == _lib.E_WORKSPACE
        assert fn(FAKE, 4, 64, 64, 3, FAKE, None, ctypes.c_void_p(4096 + 64), need, None) == _lib.E_WORKSPACE


def test_wrapper_argument_errors_come_before_the_device(monkeypatch):
    from sr_mi355x import api, psf_device

    def no_device(*a, **k):
        raise AssertionError("the wrapper touched the device before checking its arguments")

    monkeypatch.setattr(api, "_device", no_device)
    frame = np.zeros((40, 40), np.uint8)
    with pytest.raises(ValueError):
        psf_device.estimate_psf([])
    with pytest.raises(ValueError):
        psf_device.estimate_psf([frame, np.zeros((40, 41), np.uint8)])
    with pytest.raises(ValueError):
        psf_device.estimate_psf(np.zeros((40, 40), np.uint8))          # a single frame is not a stack
    with pytest.raises(ValueError):
        psf_device.estimate_psf(np.zeros((0, 40, 40), np.float64))
    for hw in (0, 8, -3, 2.5):
        with pytest.raises(ValueError):
            psf_device.estimate_psf([frame, frame], halfwidth=hw)


def test_wrapper_is_exported_and_sized_by_the_library():
    import sr_mi355x
    from sr_mi355x import psf_device
    assert sr_mi355x.estimate_psf is psf_device.estimate_psf and "estimate_psf" in sr_mi355x.__all__
    assert psf_device.workspace_bytes(1, *REF) == lib().srx_psf_estimate_workspace_bytes(1, *REF)
    assert psf_device.workspace_bytes(4, 30, 1536, 2048) == lib().srx_psf_estimate_workspace_bytes(4, 30, 1536, 2048, 3)
    # the chunk the arg-max tests take their sizes from is the library's: one (float64, uint32) partial per CHUNK_BYTES of a frame
    one, two = (lib().srx_psf_estimate_workspace_bytes(1, 1024, 1, n, 3) for n in (psf_device.CHUNK_BYTES, psf_device.CHUNK_BYTES + 1))
    assert two - one == 1024 * (8 + 4)


def test_memory_contract_cases_are_declared():
    """tests/test_memguard_host.py asks every device-output entry point of include/srx.h for a memory-contract case; those of
    srx_psf_estimate_* live in tests/test_gpu_psf.py and are registered in the same list."""
    import test_gpu_memory_contract as T
    ids = T.all_case_ids()
    assert set(test_gpu_psf.CONTRACT) <= set(ids)
    for name in ("srx_psf_estimate_u8", "srx_psf_estimate_f32", "srx_psf_estimate_f64"):
        assert any(name in i.split("-") for i in ids), name
