"""The colour entry points on the device (include/srx_bayer.h), everything bit for bit: split and mean against numpy's strided slices and
integer sums and against the four-call compositions they replace (srx_decimate_*, srx_mean_u8 per plane), the merge against the header's
numpy expressions in the working dtype, the RGB PNG file against the host's container around png_deflate's stream of the [H, 3 W] view, and
the colour reconstruction against session.reconstruct on each plane alone."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import bayer_cases as BC
import sr_mi355x as S
from sr_mi355x import _lib, api, session, synth

pytestmark = pytest.mark.gpu
CUDA = "cuda"
DT = {"f32": torch.float32, "f64": torch.float64}
PRECS = ("f32", "f64")


def frames(shape, seed):
    """seeded uint8 frames with both ends of the range present"""
    a = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    a.reshape(-1)[::7] = 255
    a.reshape(-1)[3::11] = 0
    return a


def at_offset(a, off):
    """the array on the device, its first sample `off` bytes behind a 256-byte boundary inside a larger buffer"""
    isz = a.dtype.itemsize
    assert off % isz == 0
    buf = torch.zeros(256 + off + a.nbytes + 64, dtype=torch.uint8, device=CUDA)
    start = (-buf.data_ptr()) % 256 + off
    t = buf[start:start + a.nbytes].view(torch.from_numpy(a).dtype).view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 256 == off and t.is_contiguous()
    return t


# =====================================================================================================================================
# split
# =====================================================================================================================================
@pytest.mark.parametrize("shape", BC.RAW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_u8(shape):
    H, W = shape
    for B in BC.BATCHES:
        a = frames((B, H, W), 11 * B + H)
        want = BC.split_model(a)
        for off in BC.OFFSETS:
            x = at_offset(a, off)
            got = S.bayer_split(x)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, 4, H // 2, W // 2)
            assert np.array_equal(got.cpu().numpy(), want), (B, off)
            for p, (py, px) in enumerate(BC.PLANES):
                assert torch.equal(got[:, p], S.decimate_u8(x, 2, py, px)), (B, off, p)
    assert np.array_equal(S.bayer_split(a[0]), want[0])   # numpy in, numpy out, no batch axis


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", BC.RAW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_float(shape, prec):
    H, W = shape
    t = BC.NP[prec]
    with api.precision_override(prec):
        for B in BC.BATCHES:
            a = (np.random.default_rng(5 + B).uniform(-3, 260, (B, H, W))).astype(t)
            want = BC.split_model(a)
            for off in (0, a.dtype.itemsize):   # float pointers are element aligned
                x = at_offset(a, off)
                got = S.bayer_split(x)
                assert got.dtype == DT[prec]
                assert np.array_equal(got.cpu().numpy(), want), (B, off)
                for p, (py, px) in enumerate(BC.PLANES):
                    ref = torch.stack([S.decimate(x[b], 2, py, px) for b in range(B)])
                    assert torch.equal(got[:, p], ref), (B, off, p)


# =====================================================================================================================================
# mean
# =====================================================================================================================================
@pytest.mark.parametrize("shape", BC.RAW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mean(shape):
    H, W = shape
    for B in BC.BATCHES:
        for R in BC.REPS + ((258,) if shape == (4, 8) else ()):
            a = frames((B, R, H, W), 100 * B + R + W)
            for prec in PRECS:
                want = BC.mean_model(a, prec)
                for off in BC.OFFSETS:
                    x = at_offset(a, off)
                    got = S.bayer_mean_u8(x, precision=prec)
                    assert got.dtype == DT[prec] and tuple(got.shape) == (B, 4, H // 2, W // 2)
                    assert np.array_equal(got.cpu().numpy(), want), (B, R, prec, off)
                    for p, (py, px) in enumerate(BC.PLANES):
                        assert torch.equal(got[:, p], S.mean_u8(x, 2, py, px, precision=prec)), (B, R, prec, off, p)


def test_mean_of_one_frame_is_the_split_with_conversion():
    a = frames((2, 1, 18, 34), 3)
    for prec in PRECS:
        got = S.bayer_mean_u8(torch.from_numpy(a).to(CUDA), precision=prec).cpu().numpy()
        assert np.array_equal(got, BC.split_model(a[:, 0]).astype(BC.NP[prec]))


def test_wrappers_refuse_odd_shapes_and_other_types():
    with pytest.raises(ValueError, match="even"):
        S.bayer_split(np.zeros((3, 4), np.uint8))
    with pytest.raises(ValueError, match="even"):
        S.bayer_mean_u8(np.zeros((1, 2, 4, 5), np.uint8))
    with pytest.raises(TypeError):
        S.bayer_split(np.zeros((4, 4), np.int16))
    with pytest.raises(TypeError):
        S.bayer_mean_u8(np.zeros((1, 2, 4, 4), np.float32))
    for factor in (1, 3, -2):
        with pytest.raises(ValueError, match="even factor"):
            S.bayer_merge(np.zeros((4, 2, 2)), factor)
    with pytest.raises(ValueError):
        S.bayer_merge(np.zeros((3, 2, 2)), 2)
    with pytest.raises(ValueError):
        S.png_file_rgb8(np.zeros((4, 4, 4), np.uint8))
    with pytest.raises(TypeError):
        S.png_file_rgb8(np.zeros((4, 4, 3), np.float32))


# =====================================================================================================================================
# merge
# =====================================================================================================================================
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", BC.MERGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}_d{s[2]}")
def test_merge(shape, prec):
    Hp, Wp, d = shape
    B = 2
    # samples with fractions, below 0 and above 255: sums that round in float32, and both clamps of the quantiser
    P = np.random.default_rng(Hp * Wp + d).uniform(-20, 290, (B, 4, Hp, Wp)).astype(BC.NP[prec])
    x = torch.from_numpy(P).to(CUDA)
    with api.precision_override(prec):
        for name, gains in BC.GAINS.items():
            want = BC.merge_model(P, d, gains, prec)
            got = S.bayer_merge(x, 2 * d, gains)
            assert got.dtype == DT[prec] and tuple(got.shape) == (B, 3, Hp, Wp)
            assert np.array_equal(got.cpu().numpy(), want), name
            got8 = S.bayer_merge(x, 2 * d, gains, rgb8=True)
            assert got8.dtype == torch.uint8 and tuple(got8.shape) == (B, Hp, Wp, 3)
            assert np.array_equal(got8.cpu().numpy(), BC.rgb8_model(P, d, gains, prec)), name
            assert torch.equal(got8, S.quantize_u8(got).permute(0, 2, 3, 1).contiguous()), name   # quantise-and-interleave of the planar result
        single = S.bayer_merge(x[1], 2 * d, BC.GAINS["wb"])
        assert torch.equal(single, S.bayer_merge(x, 2 * d, BC.GAINS["wb"])[1])


# =====================================================================================================================================
# RGB PNG files
# =====================================================================================================================================
def rgb_images(B, H, W, seed):
    """one smooth (compressible) and one random image per pair"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    smooth = np.stack([(30 + xx // 3 + yy) % 256, (200 - xx + 2 * yy) % 256, (xx * yy) % 256], axis=-1).astype(np.uint8)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.stack([smooth, noise][:B])


def files_of(x):
    files, lengths = S.png_file_rgb8(x)
    host, n = files.cpu().numpy(), lengths.cpu().tolist()
    assert files.shape[1] == _lib.load().srx_png_file_rgb8_bound(x.shape[-3], x.shape[-2])
    return [host[b, :n[b]].tobytes() for b in range(len(n))]


@pytest.mark.parametrize("shape", BC.PNG_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_png_file_rgb8(shape):
    H, W = shape
    img = rgb_images(2, H, W, H + W)
    x = torch.from_numpy(img).to(CUDA)
    got = files_of(x)
    streams, lengths = S.png_deflate(x.view(2, H, 3 * W))
    sh, n = streams.cpu().numpy(), lengths.cpu().tolist()
    for b in range(2):
        assert got[b] == BC.rgb_container(W, H, sh[b, :n[b]].tobytes()), b
        im = Image.open(io.BytesIO(got[b]))
        assert im.mode == "RGB" and im.size == (W, H)
        assert np.array_equal(np.asarray(im), img[b]), b
        assert files_of(x[b]) == [got[b]], b   # B = 2 is two B = 1 calls
    assert got == files_of(img)   # a host array goes the same way


# =====================================================================================================================================
# the colour reconstruction: four planes as a batch of four items under one table
# =====================================================================================================================================
def plane_frames(seed, N=4, H=64, W=64):
    """N raw frames of a smooth coloured scene with noise -> uint8 [N, 4, H/2, W/2]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    frames_ = []
    for k in range(N):
        base = 120 + 60 * np.sin(0.21 * xx + 0.4 * k) * np.cos(0.17 * yy) + rng.normal(0, 3, (H, W))
        base[0::2, 0::2] *= 1.2
        base[1::2, 1::2] *= 0.7
        frames_.append(np.clip(np.rint(base), 0, 255).astype(np.uint8))
    return BC.split_model(np.stack(frames_))


@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8"])
@pytest.mark.parametrize("prec", PRECS)
def test_reconstruct_colour_is_reconstruct_on_every_plane(prec, u8):
    pf = plane_frames(7)
    shifts, psf = np.asarray(synth.NOMINAL_4, dtype=np.float64), synth.gaussian_psf()
    with api.precision_override(prec):
        dev = torch.from_numpy(pf).to(CUDA)
        lr = [dev[k] if u8 else dev[k].to(DT[prec]) for k in range(4)]
        rgb, images, traces = session.reconstruct_colour(lr, shifts, psf, 3, 2, 0.5, gains=None)
        assert len(images) == 4 and len(traces) == 4
        for p in range(4):
            want_images, want_trace = session.reconstruct([f[p] for f in lr], shifts, psf, 3, 2, 0.5)
            assert set(images[p]) == set(want_images)
            for key in want_images:
                assert torch.equal(torch.as_tensor(images[p][key]), torch.as_tensor(want_images[key])), (p, key)
            assert np.array_equal(np.asarray(traces[p]), np.asarray(want_trace)), p
        assert set(rgb) == {"native_2x", "SAA", "SAA_IBP"}
        for key in rgb:
            assert rgb[key].dtype == torch.uint8 and tuple(rgb[key].shape) == (64, 64, 3)
            assert torch.equal(rgb[key][..., 0], S.quantize_u8(images[0][key])), key
            stacked = torch.stack([images[p][key] for p in range(4)])
            assert torch.equal(rgb[key], S.bayer_merge(stacked, 2, None, rgb8=True)), key
