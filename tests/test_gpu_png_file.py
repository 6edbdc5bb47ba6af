"""srx_png_file_* / api.png_file / api.png_encode on the GPU, and the session's device_png writer built on them.

The reference of every file is exact: bytes [0, lengths[b]) of slot b must equal session.png_container(W, H, stream), the host's wrapper
(zlib.crc32 for the chunks' CRCs) around the stream api.png_deflate returns for the same input, and PIL must open them to api.quantize_u8
of the image.  The images are those of tests/test_gpu_png.py in its three input kinds; rows of random bytes, which the coder stores, put
the IDAT's length around the CRC kernels' span and segment boundaries.

The memory-contract cases register their ids through test_gpu_memory_contract.ids (each names its entry point); the outputs of these
entry points are `void *`, so the census of tests/test_memguard_host.py does not ask for them."""
import ctypes
import io
import json
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import memguard as MG
import png_cases as PC
import test_gpu_memory_contract as T
import test_gpu_png as TP
from sr_mi355x import _lib, api, session, synth

pytestmark = pytest.mark.gpu
CUDA = "cuda"
KINDS = TP.KINDS
U8 = TP.U8
SPAN, SEGMENT, EXTRA = 64, 16384, 57


def file_call(x, kind):
    if kind == "u8":
        return api.png_file(x)
    with api.precision_override(kind):
        return api.png_file(x)


def files_of(x, kind):
    f, n = file_call(x, kind)
    f, n = f.cpu().numpy(), n.cpu().tolist()
    return [f[b, :n[b]].tobytes() for b in range(len(n))]


def check(x, kind):
    """x [B, H, W] or [H, W] of the input type `kind`: the files against png_container around png_deflate's streams of the same tensor"""
    want = TP.quantized(x, kind)
    want = want[None] if want.ndim == 2 else want
    B, H, W = want.shape
    f, n = file_call(x, kind)
    assert f.dtype == torch.uint8 and tuple(f.shape) == (B, PC.bound(H, W) + EXTRA) and n.dtype == torch.int64 and tuple(n.shape) == (B,)
    assert f.is_cuda and n.is_cuda
    streams = TP.streams_of(x, kind)
    files = files_of(x, kind)
    assert n.cpu().tolist() == [len(z) + EXTRA for z in streams]
    for b in range(B):
        assert files[b] == session.png_container(W, H, streams[b]), b
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[b]))), want[b]), b
    assert TP.encode(x, kind) == files  # png_encode is png_file, downloaded
    return files


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(U8))
def test_file_is_the_container_around_the_stream(name, kind):
    f = check(TP.as_kind(U8[name], kind), kind)[0]
    if name == "97x701_random":  # three stored chunks: a stream of 68 117 bytes, five segments of the CRC
        assert len(f) == 68117 + EXTRA
    if name == "1x1":
        assert len(f) == 15 + EXTRA


# the IDAT's CRC is the stream's under the seed crc32("IDAT"): a stored row of w random bytes is a stream of w + 14
BOUNDARY_W = [n - 14 for n in (SPAN - 1, SPAN, SPAN + 1, SEGMENT - 1, SEGMENT, SEGMENT + 1)]


@pytest.mark.parametrize("w", BOUNDARY_W)
def test_idat_lengths_around_the_span_and_the_segment(w):
    row = np.random.default_rng(w).integers(0, 256, (1, w)).astype(np.uint8)
    x = torch.from_numpy(row).to(CUDA)
    _, n = api.png_file(x)
    assert n.cpu().tolist() == [w + 14 + EXTRA]  # the premise: one stored block
    f = check(x, "u8")[0]
    assert struct.unpack(">I", f[33:37])[0] == w + 14 and f[37:41] == b"IDAT"
    assert struct.unpack(">I", f[41 + w + 14:41 + w + 18])[0] == zlib.crc32(f[37:41 + w + 14])


@pytest.mark.parametrize("kind", KINDS)
def test_batch_items_get_their_single_image_bytes_and_calls_repeat(kind):
    rng = np.random.default_rng(3)
    a = np.stack([PC.quantize(PC.truth_noise(70, 1000)), np.zeros((70, 1000), np.uint8), rng.integers(0, 256, (70, 1000)).astype(np.uint8)])
    x = TP.as_kind(a, kind)
    batch = check(x, kind)
    assert len({len(f) for f in batch}) == 3
    for b in range(3):
        assert files_of(x[b], kind)[0] == batch[b], b
    assert files_of(x, kind) == batch


# =====================================================================================================================================
# memory contract: guards around files, lengths and the workspace, a poisoned workspace, intact inputs, odd byte addresses
# =====================================================================================================================================
CONTRACT_SHAPES = {"70x1000": (2, 70, 1000), "1x1": (3, 1, 1)}
CONTRACT_IDS = [f"srx_png_file_{k}-{c}-skip{skip}" for k in KINDS for c in CONTRACT_SHAPES for skip in (0, 1)]


@pytest.mark.parametrize("cid", CONTRACT_IDS, ids=T.ids(CONTRACT_IDS))
def test_memory_contract(cid):
    entry, case, skip = cid.split("-")
    kind, skip = entry.rsplit("_", 1)[1], int(skip[4:])
    B, H, W = CONTRACT_SHAPES[case]
    rng = np.random.default_rng(17)
    a = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    if case == "70x1000":
        a[0] = 0                       # item 0 compresses (one CRC segment), item 1 is stored (five)
    x = T.put(TP.as_kind(a, kind), skip)  # skip = 1: the input one element off the 256-byte grid ...
    lib = _lib.load()
    slot = lib.srx_png_file_bound(H, W)
    files = T.out((B, slot), torch.uint8, skip=skip)  # ... and the files and their lengths at odd byte addresses
    lengths = MG.Guarded(skip + 8 * B, CUDA)
    lengths.t, lengths.skip_bytes = lengths.payload[skip:], skip
    assert files.t.data_ptr() % 2 == skip and lengths.t.data_ptr() % 2 == skip
    ws = MG.Guarded(lib.srx_png_file_scratch_bytes(B, H, W), CUDA)
    st = api._stream()
    seen = []

    def call():
        rc = getattr(lib, entry)(T.p(x), B, H, W, T.p(files.t), T.p(lengths.t), ctypes.c_void_p(ws.ptr), ws.nbytes, st)
        torch.cuda.synchronize()
        n = np.frombuffer(lengths.t.cpu().numpy().tobytes(), "<i8").tolist()
        s = files.t.cpu().numpy()
        assert all(EXTRA < n[b] <= slot for b in range(B))
        for b in range(B):  # behind the file the slot keeps what it held
            assert (s[b, n[b]:] == files.poison).all(), b
        seen.append([s[b, :n[b]].tobytes() for b in range(B)])
        return rc

    MG.run_poisoned(call, [lengths], [ws, files], [x])
    assert seen[0] == seen[1] == seen[2]
    streams = TP.streams_of(x, kind)
    assert seen[0] == [session.png_container(W, H, z) for z in streams] == files_of(x, kind)
    # a workspace one byte short or off the 256-byte grid is refused on the host and nothing is stored
    for g in (files, lengths):
        g.fill(MG.POISON_GARBAGE)
    short = MG.Guarded(ws.nbytes - 1, CUDA)
    assert getattr(lib, entry)(T.p(x), B, H, W, T.p(files.t), T.p(lengths.t), ctypes.c_void_p(short.ptr), short.nbytes, st) == _lib.E_WORKSPACE
    assert getattr(lib, entry)(T.p(x), B, H, W, T.p(files.t), T.p(lengths.t), ctypes.c_void_p(ws.ptr + 64), ws.nbytes - 64, st) == _lib.E_WORKSPACE
    assert short.untouched() and files.untouched() and lengths.untouched()


def test_wrapper_refuses_other_shapes():
    with pytest.raises(ValueError):
        api.png_file(torch.zeros((2, 2, 4, 4), dtype=torch.uint8, device=CUDA))
    with pytest.raises(ValueError):
        api.png_file(np.zeros((7,), np.uint8))
    f, n = api.png_file(np.full((4, 6), 9, np.uint8))  # numpy in: uploaded as bytes, device tensors out
    assert f.is_cuda and tuple(f.shape) == (1, PC.bound(4, 6) + EXTRA) and int(n[0]) > EXTRA


# =====================================================================================================================================
# session: device_png writes files whose container and CRCs are the host wrapper's
# =====================================================================================================================================
def _idat(data):
    """the payload of the file's one IDAT chunk, after walking the chunks"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, tags, payload = 8, [], None
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        tags.append(tag)
        if tag == b"IDAT":
            payload = data[at + 8:at + 8 + n]
        at += 12 + n
    assert at == len(data) and tags == [b"IHDR", b"IDAT", b"IEND"]
    return payload


def test_session_files_are_the_container_around_their_own_payload(tmp_path, monkeypatch):
    monkeypatch.setattr(session, "DEVICE_PNG_FILES", True)
    sess = TP._barcode_session(tmp_path / "data" / "sess0")
    psf = synth.gaussian_psf()
    outs = {flag: session.process_session(sess, psf, str(tmp_path / f"out_{int(flag)}"), kind="mono_barcodes", n_iter=3, verbose=False,
                                          device_png=flag) for flag in (False, True)}
    for d0, d1 in zip(outs[False], outs[True]):
        TP._same_outputs(d0, d1)  # the pixels of the default writer's files, convergence.json, done.flag
        for name in ("native_2x.png", "SAA.png", "SAA_IBP.png", "LR_mean.png"):
            with open(os.path.join(d1, name), "rb") as fp:
                data = fp.read()
            w, h = Image.open(io.BytesIO(data)).size
            assert data == session.png_container(w, h, _idat(data)), name
        with open(os.path.join(d1, "convergence.json")) as fp:
            assert len(json.load(fp)["ibp_mse"]) == 3


def test_session_writes_the_same_bytes_in_both_forms(tmp_path, monkeypatch):
    sess = TP._barcode_session(tmp_path / "data" / "sess0")
    psf = synth.gaussian_psf()
    outs = {}
    for files in (True, False):
        monkeypatch.setattr(session, "DEVICE_PNG_FILES", files)
        outs[files] = session.process_session(sess, psf, str(tmp_path / f"out_{int(files)}"), kind="mono_barcodes", n_iter=3, verbose=False,
                                              device_png=True)
    for d0, d1 in zip(outs[False], outs[True]):
        for name in ("native_2x.png", "SAA.png", "SAA_IBP.png", "LR_mean.png"):
            with open(os.path.join(d0, name), "rb") as f0, open(os.path.join(d1, name), "rb") as f1:
                assert f0.read() == f1.read(), name
