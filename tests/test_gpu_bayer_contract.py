"""The memory contract and the stream and graph contract of include/srx_bayer.h, entry point by entry point -- what
tests/test_gpu_memory_contract.py and tests/test_gpu_stream_contract.py hold the entry points of srx.h to, with the same two checkers.

Memory (tests/memguard.py): outputs between guard bands, srx_png_file_rgb8's scratch of exactly the queried size and poisoned, inputs
intact, every output element written (bit-identical results across the poisons, floats finite), and every pointer once on the 256-byte
grid and once only element aligned (skip = 1: a uint8 frame starting on an odd byte).

Streams (tests/streamcheck.py, through tests/bayer_stream_worker.py in a fresh child process with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 -- the
one variable tests/test_gpu_stream_contract.py sets, for the reason given there -- and no other): each call captured on a side stream queues
kernel nodes only, the documented 1, 1, 1, 1 and 5 of them, nothing runs eagerly, and the graph launched on samples it has not seen gives
the bits of a plain call."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayer_cases as BC
import bayer_stream_worker as BW
import memguard as MG
import test_gpu_memory_contract as T
from sr_mi355x import _lib, api

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U8 = torch.uint8


def st():
    return api._stream()


def host(t):
    return t.cpu().numpy()


# =====================================================================================================================================
# memory
# =====================================================================================================================================
@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
@pytest.mark.parametrize("shape", [(2, 2), (18, 34)], ids=["2x2", "18x34"])
def test_split_memory(kind, shape):
    H, W = shape
    B = 2
    fn = getattr(T.lib(), "srx_bayer_split_" + kind)
    for skip in (0, 1):
        x = T.put(T._u8((B, H, W), 71) if kind == "u8" else T.rnd((B, H, W), kind, 71, integer=False), skip)
        o = T.out((B, 4, H // 2, W // 2), x.dtype, skip)
        res = MG.run_poisoned(lambda: fn(T.p(x), B, H, W, T.p(o.t), st()), [o], (), [x], MG.INT_POISONS if kind == "u8" else MG.POISONS)
        assert np.array_equal(host(res[0]), BC.split_model(host(x))), skip


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("shape", [(2, 2), (6, 40), (18, 34)], ids=["2x2", "6x40_vectors", "18x34_samples"])
def test_mean_memory(prec, shape):
    H, W = shape
    B, R = 2, 3
    for skip in (0, 1, 3):
        x = T.put(T._u8((B, R, H, W), 72), skip)
        o = T.out((B, 4, H // 2, W // 2), T.DT[prec], min(skip, 1))
        res = MG.run_poisoned(lambda: T.lib().srx_bayer_mean_u8(T.p(x), B, R, H, W, T.EB[prec], T.p(o.t), st()), [o], (), [x])
        assert np.array_equal(host(res[0]), BC.mean_model(host(x), prec)), skip


@pytest.mark.parametrize("prec", T.PRECS)
@pytest.mark.parametrize("rgb8", [False, True], ids=["planar", "rgb8"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (21, 37, 1), (3, 5, 7)], ids=["1x1_d1", "21x37_d1", "3x5_d7"])
def test_merge_memory(shape, rgb8, prec):
    Hp, Wp, d = shape
    B = 2
    fn = T.fn("srx_bayer_merge_rgb8" if rgb8 else "srx_bayer_merge", prec)
    for skip in (0, 1):
        for gains in (None, (1.5, 1.0, 0.75)):
            x = T.put(T.rnd((B, 4, Hp, Wp), prec, 73, integer=False) * 1.2 - 20, skip)
            o = T.out((B, Hp, Wp, 3), U8, skip) if rgb8 else T.out((B, 3, Hp, Wp), T.DT[prec], skip)
            g, gp = T.hd(gains) if gains else (None, None)
            res = MG.run_poisoned(lambda: fn(T.p(x), B, Hp, Wp, d, gp, T.p(o.t), st()), [o], (), [x], MG.INT_POISONS if rgb8 else MG.POISONS)
            model = BC.rgb8_model if rgb8 else BC.merge_model
            assert np.array_equal(host(res[0]), model(host(x), d, gains, prec)), (skip, gains)


@pytest.mark.parametrize("shape", [(1, 1), (5, 43), (70, 340)], ids=["1x1", "5x43", "70x340"])
def test_png_file_rgb8_memory(shape):
    """the slots and the lengths between guard bands, the scratch of exactly srx_png_file_rgb8_scratch_bytes poisoned; a scratch one byte
    short or off the 256-byte grid is refused with nothing stored.  The slots' bytes behind a file are not documented, so what is compared
    across the poisons is the lengths and the files."""
    H, W = shape
    B = 2
    L = T.lib()
    bound, need = L.srx_png_file_rgb8_bound(H, W), L.srx_png_file_rgb8_scratch_bytes(B, H, W)
    seen = []
    for skip in (0, 1):
        x = T.put(T._u8((B, H, W, 3), 74), skip)
        slots, lengths = T.out((B, bound), U8, skip), T.out((B,), torch.int64, 0)

        def call(wp, wn):
            return L.srx_png_file_rgb8(T.p(x), B, H, W, T.p(slots.t), T.p(lengths.t), wp, wn, st())

        for poison in MG.INT_POISONS:
            ws = MG.Guarded(need, T.CUDA)
            for g in (slots, lengths, ws):
                g.fill(poison)
            before = x.clone()
            assert call(ctypes.c_void_p(ws.ptr), ctypes.c_size_t(need)) == 0
            torch.cuda.synchronize()
            for name, g in (("slots", slots), ("lengths", lengths), ("scratch", ws)):
                g.check(f"poison 0x{poison:02X}: {name}")
            assert torch.equal(x, before)
            n = lengths.t.cpu().tolist()
            assert all(57 < v <= bound for v in n)
            seen.append([host(slots.t)[b, :n[b]].tobytes() for b in range(B)])
        T.refused(call, [slots, lengths], need)
    assert all(s == seen[0] for s in seen)
    streams, slen = api.png_deflate(x.view(B, H, 3 * W))
    sh, sn = host(streams), slen.cpu().tolist()
    assert seen[0] == [BC.rgb_container(W, H, sh[b, :sn[b]].tobytes()) for b in range(B)]


# =====================================================================================================================================
# streams
# =====================================================================================================================================
def test_stream_contract():
    env = dict(os.environ, DEBUG_CLR_GRAPH_PACKET_CAPTURE="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "bayer_stream_worker.py")], env=env, capture_output=True, text=True, timeout=120)
    lines = r.stdout.strip().splitlines()
    assert lines, f"the worker printed nothing (exit status {r.returncode}): {r.stderr[-2000:]}"
    res = json.loads(lines[-1])
    for cid, v in res.items():
        print(f"{cid}: {v['nodes']}" + (f"  -- {v['detail']}" if v["detail"] else ""))
    bad = {k: v["detail"] for k, v in res.items() if not v["ok"]}
    assert not bad, bad
    assert list(res) == list(BW.CASES), f"the worker stopped early or ran other cases (exit status {r.returncode}): {r.stderr[-2000:]}"
    assert r.returncode == 0, r.stderr[-2000:]
    for cid, (_, kernels) in BW.CASES.items():
        assert res[cid]["nodes"]["kernel"] == kernels and res[cid]["nodes"]["memcpy"] == 0, cid


def test_the_stream_cases_name_every_entry_point():
    called = {n for n in _lib.bayer_symbols() if not n.endswith(("_bound", "_scratch_bytes"))}
    assert {cid.split("-")[0] for cid in BW.CASES} == called
