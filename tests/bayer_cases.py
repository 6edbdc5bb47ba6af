"""numpy models and shape lists of the colour entry points (include/srx_bayer.h), shared by tests/test_bayer_host.py,
tests/test_gpu_bayer.py, tests/test_gpu_bayer_contract.py and tests/bayer_stream_worker.py.  A plain helper module: numpy only.

Plane p = 0..3 is R, G1, G2, B: raw[py::2, px::2] with (py, px) = (p >> 1, p & 1)."""
import struct
import zlib

import numpy as np

NP = {"f32": np.float32, "f64": np.float64}
PLANES = [(p >> 1, p & 1) for p in range(4)]

# raw (H, W): the smallest; H W a multiple of 16 with a row shorter than a vector; H W a multiple of 16 and W not (every row cut differently);
# neither (the sample-by-sample kernel); rows of whole vectors
RAW_SHAPES = [(2, 2), (4, 8), (6, 40), (18, 34), (32, 64)]
OFFSETS = (0, 1, 3, 15)          # bytes between a 256-byte boundary and the raw stack's first sample
BATCHES = (1, 3)
REPS = (1, 2, 5)                 # and 258 at 4 x 8 only: it crosses a packed group (257 frames)
MERGE_SHAPES = [(2, 2, 1), (4, 6, 1), (8, 8, 2), (8, 8, 0), (66, 130, 1), (3, 5, 7)]   # (Hp, Wp, d); the last: every index clamps
GAINS = {"none": None, "ones": (1.0, 1.0, 1.0), "wb": (1.5, 1.0, 0.75)}
PNG_SHAPES = [(1, 1), (5, 43), (64, 200)]   # 64 x 601 scanline bytes cross the 32 KB chunk


def split_model(raw):
    """raw [..., H, W] -> [..., 4, H/2, W/2]: strided slices"""
    return np.stack([raw[..., py::2, px::2] for py, px in PLANES], axis=-3)


def mean_model(stack, prec):
    """uint8 [B, R, H, W] -> [B, 4, H/2, W/2]: an integer sum and one division in the working dtype"""
    T = NP[prec]
    s = stack.astype(np.int64).sum(axis=1)
    return split_model(s.astype(T) / T(stack.shape[1]))


def merge_model(planes, d, gains, prec):
    """planes [B, 4, Hp, Wp] -> rgb [B, 3, Hp, Wp], every operation in the working dtype (include/srx_bayer.h gives the expressions)"""
    T = NP[prec]
    P = np.asarray(planes, dtype=T)
    Hp, Wp = P.shape[-2:]
    yc, xc = np.clip(np.arange(Hp) - d, 0, Hp - 1), np.clip(np.arange(Wp) - d, 0, Wp - 1)
    R = P[:, 0]
    G = (P[:, 1][:, :, xc] + P[:, 2][:, yc, :]) * T(0.5)
    Bl = P[:, 3][:, yc][:, :, xc]
    rgb = np.stack([R, G, Bl], axis=1)
    if gains is not None:
        rgb = rgb * np.asarray(gains, dtype=np.float64).astype(T)[None, :, None, None]
    assert rgb.dtype == T
    return rgb


def quantize_model(x):
    """np.clip(x, 0, 255).astype(np.uint8): srx_quantize_u8_T"""
    return np.clip(x, 0, 255).astype(np.uint8)


def rgb8_model(planes, d, gains, prec):
    """-> uint8 [B, Hp, Wp, 3]: the planar result quantised and interleaved"""
    return np.ascontiguousarray(quantize_model(merge_model(planes, d, gains, prec)).transpose(0, 2, 3, 1))


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def rgb_container(W, H, stream):
    """signature + truecolour IHDR + one IDAT around `stream` + IEND"""
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) + chunk(b"IDAT", bytes(stream)) + chunk(b"IEND", b""))
