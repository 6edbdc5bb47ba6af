"""srx_png_deflate_* / api.png_deflate / api.png_encode on the GPU, and the session option built on them (device_png, run_sr --png-on-device).

The reference of every stream is exact: zlib.decompress of bytes [0, lengths[b]) of slot b must equal the Up-filtered scanlines of
api.quantize_u8 of the image (tests/png_cases.py), PIL must open png_encode's files to the same pixels, and lengths[b] stays within
srx_png_stream_bound.  The images are those of tests/test_png_host.py (the smallest shapes at which each piece of the coder can go wrong),
each as uint8, float32 and float64 (the float forms carry a fraction that the quantiser must truncate).  Two size caps against the host
writer's own zlib stream keep a valid but useless coder (everything stored) from passing.

The memory-contract cases register their ids through test_gpu_memory_contract.ids (each names its entry point); the outputs of these
entry points are `void *`, so the census of tests/test_memguard_host.py does not ask for them."""
import ctypes
import io
import json
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import memguard as MG
import png_cases as PC
import test_gpu_memory_contract as T
from sr_mi355x import _lib, api, run_sr, session, synth

pytestmark = pytest.mark.gpu
CUDA = "cuda"
KINDS = ("u8", "f32", "f64")
U8 = PC.u8_cases()


def as_kind(a_u8, kind):
    """a uint8 image as the tensor of an input type; the float forms sit 0.37 above the integer (255.37 is the clamp's to bring back)"""
    t = torch.from_numpy(np.ascontiguousarray(a_u8)).to(CUDA)
    if kind == "u8":
        return t
    return t.to(T.DT[kind]) + 0.37


def quantized(x, kind):
    if kind == "u8":
        return x.cpu().numpy()
    with api.precision_override(kind):
        return api.quantize_u8(x).cpu().numpy()


def deflate(x, kind):
    if kind == "u8":
        return api.png_deflate(x)
    with api.precision_override(kind):
        return api.png_deflate(x)


def encode(x, kind):
    if kind == "u8":
        return api.png_encode(x)
    with api.precision_override(kind):
        return api.png_encode(x)


def streams_of(x, kind):
    s, n = deflate(x, kind)
    s, n = s.cpu().numpy(), n.cpu().tolist()
    return [s[b, :n[b]].tobytes() for b in range(len(n))]


def check(x, kind):
    """x [B, H, W] or [H, W] of the input type `kind`: streams, files and lengths against quantize_u8 of the same tensor"""
    want = quantized(x, kind)
    want = want[None] if want.ndim == 2 else want
    B, H, W = want.shape
    s, n = deflate(x, kind)
    assert s.dtype == torch.uint8 and tuple(s.shape) == (B, PC.bound(H, W)) and n.dtype == torch.int64 and tuple(n.shape) == (B,)
    assert s.is_cuda and n.is_cuda
    z = streams_of(x, kind)
    files = encode(x, kind)
    for b in range(B):
        assert 0 < len(z[b]) <= PC.bound(H, W)
        assert z[b][:2] == b"\x78\x01" and zlib.decompress(z[b]) == PC.scanlines(want[b]), b
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[b]))), want[b]), b
    return z


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(U8))
def test_stream_inflates_to_the_scanlines(name, kind):
    z = check(as_kind(U8[name], kind), kind)[0]
    raw = PC.scanlines(U8[name])
    if name == "97x701_random":  # incompressible: every chunk stored, 5 bytes each
        assert len(z) == 2 + len(raw) + 5 * 3 + 6
    if name == "1x1":
        assert len(z) == 2 + 5 + 2 + 6
    if name == "70x1000_zero":
        assert len(z) <= 0.03 * len(raw)
    if name == "truth_192x256":
        assert len(z) <= 1.05 * len(PC.host_stream(U8[name]))


@pytest.mark.parametrize("kind", ("f32", "f64"))
def test_float_inputs_quantise_like_quantize_u8(kind):
    plane = torch.from_numpy(PC.float_plane()).to(CUDA, T.DT[kind])
    check(plane, kind)
    want = quantized(plane, kind)
    assert want[0, :7].tolist() == [0, 0, 0, 0, 254, 255, 255]
    noisy = torch.from_numpy(PC.truth_noise()).to(CUDA, T.DT[kind])  # real statistics with clipped regions, never rounded to integers
    z = check(noisy, kind)[0]
    assert len(z) <= 1.05 * len(PC.host_stream(quantized(noisy, kind)))
    assert (quantized(noisy, kind) == 0).any() and (quantized(noisy, kind) == 255).mean() > 0.01  # both clamps act


def test_device_stream_is_the_host_model_s(tmp_path):
    """the kernels and tests/png_host_model.cpp run the same integer code in the same order: the same bytes"""
    import shutil
    import subprocess
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "model")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I" + os.path.join(root, "enph459-super-resolution_amd", "csrc"), "-o", exe,
                           os.path.join(root, "tests", "png_host_model.cpp")])
    for name in ("truth_192x256", "limiter_row", "70x1000_zero", "2x32767"):
        src, dst = str(tmp_path / "raw.bin"), str(tmp_path / "z.bin")
        with open(src, "wb") as fp:
            fp.write(PC.scanlines(U8[name]))
        subprocess.check_call([exe, src, dst], stdout=subprocess.DEVNULL)
        with open(dst, "rb") as fp:
            assert fp.read() == streams_of(as_kind(U8[name], "u8"), "u8")[0], name


@pytest.mark.parametrize("kind", KINDS)
def test_batch_items_get_their_single_image_bytes_and_calls_repeat(kind):
    rng = np.random.default_rng(3)
    a = np.stack([PC.quantize(PC.truth_noise(70, 1000)), np.zeros((70, 1000), np.uint8), rng.integers(0, 256, (70, 1000)).astype(np.uint8)])
    x = as_kind(a, kind)
    batch = check(x, kind)
    assert len({len(z) for z in batch}) == 3
    for b in range(3):
        assert streams_of(x[b], kind)[0] == batch[b], b
    assert streams_of(x, kind) == batch


# =====================================================================================================================================
# memory contract: guards around streams, lengths and the workspace, a poisoned workspace, intact inputs
# =====================================================================================================================================
CONTRACT_SHAPES = {"70x1000": (2, 70, 1000), "97x701": (1, 97, 701), "1x1": (3, 1, 1)}
CONTRACT_IDS = [f"srx_png_deflate_{k}-{c}-skip{skip}" for k in KINDS for c in CONTRACT_SHAPES for skip in (0, 1)]


@pytest.mark.parametrize("cid", CONTRACT_IDS, ids=T.ids(CONTRACT_IDS))
def test_memory_contract(cid):
    entry, case, skip = cid.split("-")
    kind, skip = entry.rsplit("_", 1)[1], int(skip[4:])
    B, H, W = CONTRACT_SHAPES[case]
    rng = np.random.default_rng(17)
    a = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    if case == "70x1000":
        a[0] = 0                      # item 0 compresses (Huffman chunks), item 1 is stored
    x = T.put(as_kind(a, kind), skip)  # skip = 1: the input one element (uint8: one byte) off the 256-byte grid
    assert x.data_ptr() % 256 == skip * x.element_size()
    lib = _lib.load()
    slot = lib.srx_png_stream_bound(H, W)
    streams, lengths = T.out((B, slot), torch.uint8), T.out((B,), torch.int64)
    ws = MG.Guarded(lib.srx_png_scratch_bytes(B, H, W), CUDA)
    st = api._stream()
    seen = []

    def call():
        rc = getattr(lib, entry)(T.p(x), B, H, W, T.p(streams.t), T.p(lengths.t), ctypes.c_void_p(ws.ptr), ws.nbytes, st)
        torch.cuda.synchronize()
        n = lengths.t.cpu().tolist()
        s = streams.t.cpu().numpy()
        assert all(0 < n[b] <= slot for b in range(B))
        for b in range(B):  # behind the stream the slot keeps what it held
            assert (s[b, n[b]:] == streams.poison).all(), b
        seen.append([s[b, :n[b]].tobytes() for b in range(B)])
        return rc

    # the slots are poisoned and guarded like a workspace (their tails are not the call's to write, so whole slots differ across
    # poisons); what the call did write is compared across the poisons here
    MG.run_poisoned(call, [lengths], [ws, streams], [x])
    assert seen[0] == seen[1] == seen[2]
    want = quantized(x, kind)
    for b in range(B):
        assert zlib.decompress(seen[0][b]) == PC.scanlines(want[b])
    assert seen[0] == streams_of(x, kind)


def test_wrapper_refuses_other_shapes():
    with pytest.raises(ValueError):
        api.png_deflate(torch.zeros((2, 2, 4, 4), dtype=torch.uint8, device=CUDA))
    with pytest.raises(ValueError):
        api.png_deflate(np.zeros((7,), np.uint8))
    s, n = api.png_deflate(np.full((4, 6), 9, np.uint8))  # numpy in: uploaded as bytes, device tensors out
    assert s.is_cuda and tuple(s.shape) == (1, PC.bound(4, 6)) and int(n[0]) > 0


# =====================================================================================================================================
# session: device_png writes the same pixels, the same convergence.json and done.flag; run_sr --png-on-device
# =====================================================================================================================================
def _barcode_session(root, reps=2, seed=31):
    """a synthetic mono_barcodes session: corner{c}_rep{rr}.png, 40 x 56 frames"""
    root.mkdir(parents=True)
    base = synth.truth_image(48, 64, seed=seed)
    for r in range(reps):
        for c in range(4):
            fr = synth.sensor_frames(np.roll(base, (c % 2, c // 2), axis=(0, 1))[4:44, 4:60], seed=seed + 8 * c + r).astype(np.uint8)
            session.write_png_u8(str(root / f"corner{c}_rep{r:02d}.png"), fr)
    return str(root)


def _same_outputs(d0, d1):
    names = sorted(os.listdir(d0))
    assert names == sorted(os.listdir(d1)) and "done.flag" in names and "convergence.json" in names
    pngs = [n for n in names if n.endswith(".png")]
    assert set(pngs) == {"native_2x.png", "SAA.png", "SAA_IBP.png", "LR_mean.png"}
    for n in pngs:
        a, b = np.asarray(Image.open(os.path.join(d0, n))), np.asarray(Image.open(os.path.join(d1, n)))
        assert a.dtype == b.dtype == np.uint8 and np.array_equal(a, b), n
    with open(os.path.join(d0, "convergence.json")) as f0, open(os.path.join(d1, "convergence.json")) as f1:
        assert json.load(f0) == json.load(f1)


def test_session_writes_the_same_pixels_with_device_png(tmp_path):
    sess = _barcode_session(tmp_path / "data" / "sess0")
    psf = synth.gaussian_psf()
    outs = {}
    for flag in (False, True):
        outs[flag] = session.process_session(sess, psf, str(tmp_path / f"out_{int(flag)}"), kind="mono_barcodes", n_iter=3, verbose=False,
                                             device_png=flag)
        assert [os.path.basename(d) for d in outs[flag]] == ["rep0", "rep1"]
    for d0, d1 in zip(outs[False], outs[True]):
        _same_outputs(d0, d1)
    # the default is the host writer: byte-identical files with the flag left out
    again = session.process_session(sess, psf, str(tmp_path / "out_default"), kind="mono_barcodes", n_iter=3, verbose=False)
    for d0, d2 in zip(outs[False], again):
        for n in ("SAA.png", "LR_mean.png"):
            with open(os.path.join(d0, n), "rb") as f0, open(os.path.join(d2, n), "rb") as f2:
                assert f0.read() == f2.read()


def test_run_sr_png_on_device(tmp_path, capsys):
    _barcode_session(tmp_path / "data" / "sess0", reps=1)
    try:
        for k, extra in enumerate(([], ["--png-on-device"])):
            run_sr.main(["--kind", "mono_barcodes", "--data-dir", str(tmp_path / "data"), "--output-dir", str(tmp_path / f"out{k}")] + extra)
    finally:
        api.set_precision("f32")
    capsys.readouterr()
    _same_outputs(str(tmp_path / "out0" / "sess0" / "rep0"), str(tmp_path / "out1" / "sess0" / "rep0"))
