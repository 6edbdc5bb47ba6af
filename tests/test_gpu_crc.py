"""srx_crc32 / api.crc32 on the GPU.  The reference is exact: zlib.crc32 of the same bytes under the same seed.

The lengths are the ones at which a piece of the two kernels changes its path (tests/test_crc_host.py runs the host model at the same ones):
nothing, less than a word, one span of SRX_CRC_SPAN bytes more or less a byte, one segment of SRX_CRC_SEGMENT bytes more or less a byte, three
segments whose first holds one span and a byte, and 300 001 bytes (19 segments, the first short); each with the data 0..3 bytes off a
256-byte boundary, so that the kernel's own alignment of its 16-byte loads is exercised at every head length mod 4.

The memory-contract cases register their ids through test_gpu_memory_contract.ids; the outputs of this entry point are `void *`, so the
census of tests/test_memguard_host.py does not ask for them."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import memguard as MG
import test_gpu_memory_contract as T
from sr_mi355x import _lib, api

pytestmark = pytest.mark.gpu
CUDA = "cuda"
SPAN, SEGMENT = 64, 16384
SEEDS = (0, zlib.crc32(b"IDAT"), 0xFFFFFFFF)
LENGTHS = [0, 1, 2, 3, 4, 5, SPAN - 1, SPAN, SPAN + 1, SEGMENT - 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + SPAN + 1, 300001]
BATCH_LENGTHS = [0, 1, SEGMENT, SEGMENT + 1, 2 * SEGMENT + SPAN + 1]


@pytest.fixture(scope="module")
def blob():
    """300 001 + 3 random bytes on a 256-byte boundary of the device, and the same bytes on the host"""
    host = np.random.default_rng(23).integers(0, 256, LENGTHS[-1] + 3).astype(np.uint8)
    g = MG.Guarded(host.size, CUDA)
    g.payload.copy_(torch.from_numpy(host))
    assert g.ptr % 256 == 0
    return g, host.tobytes()


def raw_call(ptr, B, stride, max_len, lengths, seed, crc, ws):
    return _lib.load().srx_crc32(ctypes.c_void_p(ptr), B, stride, max_len, None if lengths is None else T.p(lengths), seed, T.p(crc),
                                 ctypes.c_void_p(ws.data_ptr()), ws.numel(), api._stream())


def u32(t):
    return [v & 0xFFFFFFFF for v in t.cpu().tolist()]


def test_constants():
    lib = _lib.load()
    assert lib.srx_crc32_scratch_bytes(1, SEGMENT) == lib.srx_crc32_scratch_bytes(1, 1) == 256
    assert lib.srx_crc32_scratch_bytes(1, 64 * SEGMENT + 1) == 512  # 65 segments of four bytes each


def test_lengths_offsets_and_seeds_against_zlib(blob):
    g, host = blob
    cases = [(n, off, seed) for n in LENGTHS for off in range(4) for seed in SEEDS if n > 0]
    crc = torch.zeros(len(cases), dtype=torch.int32, device=CUDA)
    ws = torch.empty(_lib.load().srx_crc32_scratch_bytes(1, LENGTHS[-1]), dtype=torch.uint8, device=CUDA)
    for i, (n, off, seed) in enumerate(cases):  # max_len = n, lengths = NULL
        assert raw_call(g.ptr + off, 1, n, n, None, seed, crc[i:], ws) == _lib.OK
    got = u32(crc)
    for i, (n, off, seed) in enumerate(cases):
        assert got[i] == zlib.crc32(host[off:off + n], seed), (n, off, seed)
    # ... and every length, 0 included, as lengths[0] of a call sized for the longest
    lens = torch.tensor(LENGTHS, dtype=torch.int64, device=CUDA)
    crc = torch.zeros((4, len(SEEDS), len(LENGTHS)), dtype=torch.int32, device=CUDA)
    for off in range(4):
        for k, seed in enumerate(SEEDS):
            for i in range(len(LENGTHS)):
                assert raw_call(g.ptr + off, 1, LENGTHS[-1], LENGTHS[-1], lens[i:], seed, crc[off, k, i:], ws) == _lib.OK
    got = crc.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    for off in range(4):
        for k, seed in enumerate(SEEDS):
            for i, n in enumerate(LENGTHS):
                assert int(got[off, k, i]) == zlib.crc32(host[off:off + n], seed), (n, off, seed)


def _batch(poison, stride):
    """five items of BATCH_LENGTHS at an odd stride; every byte that belongs to no item holds `poison`"""
    rng = np.random.default_rng(41)
    a = np.full((len(BATCH_LENGTHS), stride), poison, np.uint8)
    for b, n in enumerate(BATCH_LENGTHS):
        a[b, :n] = rng.integers(0, 256, n)
    return a


@pytest.mark.parametrize("seed", SEEDS)
def test_a_batch_with_device_lengths_and_an_odd_stride(seed):
    max_len = BATCH_LENGTHS[-1]
    stride = max_len + 2
    assert stride % 2 == 1
    B = len(BATCH_LENGTHS)
    lib = _lib.load()
    ws = torch.empty(lib.srx_crc32_scratch_bytes(B, max_len), dtype=torch.uint8, device=CUDA)
    lens = torch.tensor(BATCH_LENGTHS, dtype=torch.int64, device=CUDA)
    seen = []
    for poison in (0x00, 0xA5):  # what stands at and behind lengths[b] never reaches the result
        a = _batch(poison, stride)
        buf = torch.zeros(1 + a.size, dtype=torch.uint8, device=CUDA)
        buf[1:] = torch.from_numpy(a.reshape(-1)).to(CUDA)  # one byte off the allocation's alignment
        crc = torch.zeros(B, dtype=torch.int32, device=CUDA)
        assert raw_call(buf.data_ptr() + 1, B, stride, max_len, lens, seed, crc, ws) == _lib.OK
        seen.append(u32(crc))
        assert seen[-1] == [zlib.crc32(a[b, :n].tobytes(), seed) for b, n in enumerate(BATCH_LENGTHS)]
        again = torch.zeros(B, dtype=torch.int32, device=CUDA)
        assert raw_call(buf.data_ptr() + 1, B, stride, max_len, lens, seed, again, ws) == _lib.OK
        assert u32(again) == seen[-1]  # a repeated call repeats
        one = torch.zeros(B, dtype=torch.int32, device=CUDA)
        for b in range(B):  # item b of the batch is its B = 1 call
            assert raw_call(buf.data_ptr() + 1 + b * stride, 1, stride, max_len, lens[b:], seed, one[b:], ws) == _lib.OK
        assert u32(one) == seen[-1]
        # lengths = NULL: every item is max_len long, poison included
        full = torch.zeros(B, dtype=torch.int32, device=CUDA)
        assert raw_call(buf.data_ptr() + 1, B, stride, max_len, None, seed, full, ws) == _lib.OK
        assert u32(full) == [zlib.crc32(a[b, :max_len].tobytes(), seed) for b in range(B)]
        # lengths beyond max_len clamp to it; lengths below zero are empty items
        odd = torch.tensor([max_len + 1, 1 << 40, -1, -(1 << 40), max_len], dtype=torch.int64, device=CUDA)
        clamped = torch.zeros(B, dtype=torch.int32, device=CUDA)
        assert raw_call(buf.data_ptr() + 1, B, stride, max_len, odd, seed, clamped, ws) == _lib.OK
        want = u32(full)
        assert u32(clamped) == [want[0], want[1], seed, seed, want[4]]
    assert seen[0] == seen[1]


def test_wrapper():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (3, SEGMENT + 77)).astype(np.uint8)
    got = api.crc32(torch.from_numpy(a).to(CUDA))
    assert got.is_cuda and got.dtype == torch.int64 and tuple(got.shape) == (3,)
    assert got.tolist() == [zlib.crc32(a[b].tobytes()) for b in range(3)]
    lens = [0, 5, SEGMENT + 1]
    got = api.crc32(a, lengths=lens, seed=SEEDS[1])  # numpy in: uploaded, a device tensor out
    assert got.is_cuda and got.tolist() == [zlib.crc32(a[b, :n].tobytes(), SEEDS[1]) for b, n in enumerate(lens)]
    assert api.crc32(a[0]).tolist() == [zlib.crc32(a[0].tobytes())]
    assert api.crc32(np.zeros((2, 0), np.uint8), seed=7).tolist() == [7, 7]
    for bad in (np.zeros((2, 2, 2), np.uint8), np.zeros((4,), np.float32)):
        with pytest.raises(ValueError):
            api.crc32(bad)
    with pytest.raises(ValueError):
        api.crc32(a, lengths=[1, 2])
    with pytest.raises(ValueError):
        api.crc32(a, seed=-1)


# =====================================================================================================================================
# memory contract: guards around crc and the workspace, a poisoned workspace, intact inputs
# =====================================================================================================================================
CONTRACT_IDS = [f"srx_crc32-{c}-off{off}" for c in ("batch5", "one300001") for off in (0, 3)]


@pytest.mark.parametrize("cid", CONTRACT_IDS, ids=T.ids(CONTRACT_IDS))
def test_memory_contract(cid, blob):
    _, case, off = cid.split("-")
    off = int(off[3:])
    lib = _lib.load()
    if case == "batch5":
        max_len = BATCH_LENGTHS[-1]
        B, stride, lens_host = len(BATCH_LENGTHS), max_len + 2, BATCH_LENGTHS
        a = _batch(0x3C, stride)
        x = T.put(torch.from_numpy(np.concatenate([np.zeros(off, np.uint8), a.reshape(-1)])).to(CUDA))  # ends where the guard begins
        items = [a[b, :n].tobytes() for b, n in enumerate(lens_host)]
    else:
        g, host = blob
        B, stride, max_len, lens_host = 1, LENGTHS[-1], LENGTHS[-1], [LENGTHS[-1]]
        x = g.payload[:off + max_len]
        items = [host[off:off + max_len]]
    lens = torch.tensor(lens_host, dtype=torch.int64, device=CUDA)
    crc = T.out((B,), torch.int32)
    need = lib.srx_crc32_scratch_bytes(B, max_len)
    seed = SEEDS[1]

    def call(wsp, wsn):
        return lib.srx_crc32(ctypes.c_void_p(x.data_ptr() + off), B, stride, max_len, T.p(lens), seed, T.p(crc.t), wsp, wsn, api._stream())

    res = T.contract(call, [crc], need, inputs=[x, lens])
    assert u32(res[0]) == [zlib.crc32(it, seed) for it in items]
