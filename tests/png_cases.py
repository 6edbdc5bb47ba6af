"""The images tests/test_png_host.py and tests/test_gpu_png.py encode, and the references they compare with.  A plain helper module like
ssim_oracle.py: no fixtures, nothing registered."""
import zlib

import numpy as np

from sr_mi355x import synth

CHUNK = 32768


def scanlines(a):
    """the bytes session.write_png_u8 hands to zlib for a 2-D uint8 array: H rows of filter byte 2 (Up) + the row minus the one above"""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    h, w = a.shape
    raw = np.empty((h, w + 1), np.uint8)
    raw[:, 0] = 2
    raw[0, 1:] = a[0]
    np.subtract(a[1:], a[:-1], out=raw[1:, 1:])
    return raw.tobytes()


def host_stream(a):
    """write_png_u8's own zlib stream of the same scanlines (level 1, Z_RLE)"""
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return c.compress(scanlines(a)) + c.flush()


def bound(h, w):
    raw = h * (w + 1)
    return 2 + raw + 5 * -(-raw // CHUNK) + 6


def limiter_counts(terms=18):
    """1, 2, 4, 7, 12, 20, ...: c_n = c_{n-1} + c_{n-2} + 1"""
    c = [1, 2]
    while len(c) < terms:
        c.append(c[-1] + c[-2] + 1)
    return c


def limiter_row():
    """1 x 17690: value v occurs limiter_counts()[v] times; the most frequent value on the even positions, so no two neighbours are equal.
    (Eighteen terms of the recurrence sum to 17690 -- 1, 3, 7, 14, 26, ... 6746, 10926, 17690 -- not to the 17699 the feature request
    quotes; the recurrence is what makes the unlimited code deeper than 15, so the row follows it.)"""
    c = limiter_counts()
    n = sum(c)
    assert n == 17690 and c[-1] <= (n + 1) // 2
    # the values in the order of falling counts, dealt to the even positions first and then to the odd ones: equal values end up two
    # apart (no count exceeds half the row)
    seq = np.repeat(np.arange(len(c) - 1, -1, -1, dtype=np.uint8), c[::-1])
    row = np.empty(n, np.uint8)
    row[np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])] = seq
    assert not (row[1:] == row[:-1]).any()
    assert np.array_equal(np.bincount(row, minlength=len(c)), c)
    return row.reshape(1, n)


def runs_row():
    """one row holding runs of exactly these lengths, separated by distinct values"""
    parts, v = [], 10
    for L in (2, 3, 4, 257, 258, 259, 260, 261, 516, 517):
        parts += [np.full(L, v, np.uint8), np.array([v + 101, v + 53], np.uint8)]
        v += 7
    return np.concatenate(parts).reshape(1, -1)


def truth_noise(h=192, w=256):
    """synth.truth_image plus N(0, 1) noise, scaled x 2 - 60 (clipped regions at both ends), as float64"""
    rng = np.random.default_rng(11)
    return (synth.truth_image(h, w, seed=3) + rng.normal(0.0, 1.0, (h, w))) * 2.0 - 60.0


def quantize(a):
    return np.clip(a, 0, 255).astype(np.uint8)


def u8_cases():
    rng = np.random.default_rng(5)
    bars = np.zeros((200, 300), np.uint8)
    bars[:, (np.arange(300) % 7) < 2] = 255
    return {
        "1x1": np.array([[137]], np.uint8),
        "3x5_small_values": rng.integers(0, 3, (3, 5)).astype(np.uint8),
        "70x1000_zero": np.zeros((70, 1000), np.uint8),
        "2x32767": rng.integers(0, 4, (2, 32767)).astype(np.uint8),
        "2x32766": rng.integers(0, 4, (2, 32766)).astype(np.uint8),
        "97x701_random": rng.integers(0, 256, (97, 701)).astype(np.uint8),
        "runs_row": runs_row(),
        "200x300_bars": bars,
        "limiter_row": limiter_row(),
        "truth_192x256": quantize(truth_noise()),
    }


def float_plane():
    """-3.5, -0.0, 0.0, 0.999, 254.999, 255.0, 300.0 and fractional values, 9 x 31"""
    rng = np.random.default_rng(13)
    a = rng.uniform(-20.0, 280.0, (9, 31))
    a[0, :7] = [-3.5, -0.0, 0.0, 0.999, 254.999, 255.0, 300.0]
    a[4, 3:10] = [0.5, 1.0, 1.999999, 127.5, 254.0, 255.999, 256.0]
    return a
