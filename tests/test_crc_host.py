"""srx_crc32 and srx_png_file_* without a GPU.

1. The plain integer part of csrc/srx_crc.hpp (byte table, raw of a span, gfmul, the powers x^(8 2^j), segment and slice geometry, the
   seed term) compiled for the host: tests/crc_host_model.cpp reduces a file of bytes in the kernels' order, built with
   g++ -fsanitize=address,undefined and run as a program.  Its CRC must be zlib.crc32's and no sanitizer report may appear.
2. The argument checks and refusals of the four entry points (decided on the host before any HIP call: the pointers are never
   dereferenced) and the size queries."""
import ctypes
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import png_cases as PC
import sr_mi355x
from sr_mi355x import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "enph459-super-resolution_amd", "csrc")
GXX = shutil.which("g++")

SPAN, SEGMENT = 64, 16384  # SRX_CRC_SPAN, SRX_CRC_SEGMENT (test_constants_are_the_header_s)
SEEDS = (0, zlib.crc32(b"IDAT"), 0xFFFFFFFF)


def lengths_for(span, segment):
    return [0, 1, 2, 3, 4, 5, span - 1, span, span + 1, segment - 1, segment, segment + 1, 2 * segment + span + 1, 300001]


def contents(n, kind):
    if kind == "random":
        return np.random.default_rng(n + 1).integers(0, 256, n).astype(np.uint8).tobytes()
    return bytes([0 if kind == "zeros" else 0xFF]) * n


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if GXX is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("crc_model") / "crc_host_model")
    subprocess.check_call([GXX, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "crc_host_model.cpp")])
    return exe


def model_crc(model, tmp_path, data, seed, sizes=()):
    src = str(tmp_path / "msg.bin")
    with open(src, "wb") as fp:
        fp.write(data)
    r = subprocess.run([model, src, str(seed)] + [str(v) for v in sizes], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr[-3000:]}"
    words = r.stdout.split()
    info = {words[i]: int(words[i + 1]) for i in range(0, len(words), 2)}
    return info["crc"], info["segments"]


@pytest.mark.parametrize("kind", ("random", "zeros", "ones"))
def test_model_is_zlib_crc32_at_the_kernels_sizes(model, tmp_path, kind):
    for n in lengths_for(SPAN, SEGMENT):
        data = contents(n, kind)
        for seed in SEEDS:
            got, nseg = model_crc(model, tmp_path, data, seed)
            assert got == zlib.crc32(data, seed), (n, seed)
            assert nseg == -(-n // SEGMENT)


@pytest.mark.parametrize("span,segment", [(1, 4), (3, 96), (64, 256)])
def test_model_at_other_span_and_segment_sizes(model, tmp_path, span, segment):
    """(1, 4): 75 001 segments, 293 to a slice of the finish; (3, 96): neither a power of two"""
    for n in sorted(set(lengths_for(span, segment) + lengths_for(SPAN, SEGMENT))):
        for kind in ("random", "zeros", "ones"):
            data = contents(n, kind)
            for seed in SEEDS:
                assert model_crc(model, tmp_path, data, seed, (span, segment))[0] == zlib.crc32(data, seed), (n, kind, seed)


def test_constants_are_the_header_s():
    import re
    text = open(os.path.join(ROOT, "include", "srx.h")).read()
    assert int(re.search(r"#define SRX_CRC_SPAN (\d+)", text).group(1)) == SPAN
    assert int(re.search(r"#define SRX_CRC_SEGMENT (\d+)", text).group(1)) == SEGMENT
    assert int(re.search(r"#define SRX_PNG_FILE_EXTRA (\d+)", text).group(1)) == 57
    src = open(os.path.join(CSRC, "srx_crc.hpp")).read()
    assert f"constexpr int SPAN = {SPAN};" in src and f"constexpr int SEGMENT = {SEGMENT};" in src


# ---------------------------------------------------------------------------------------------------------------------------------
# entry points: refusals and queries
# ---------------------------------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)
CRC_OK = dict(data=FAKE, B=1, stride=100, max_len=100, lengths=FAKE, seed=0, crc=FAKE, ws=FAKE, wsb=1 << 20)


def crc_call(**kw):
    a = dict(CRC_OK, **kw)
    return _lib.load().srx_crc32(a["data"], a["B"], a["stride"], a["max_len"], a["lengths"], a["seed"], a["crc"], a["ws"], a["wsb"], None)


CRC_INVALID = {"null_data": dict(data=None), "null_crc": dict(crc=None), "B0": dict(B=0), "B_neg": dict(B=-1), "max_len0": dict(max_len=0),
               "short_stride": dict(B=2, stride=99), "lengths_off_8": dict(lengths=ctypes.c_void_p(4096 + 4)),
               "crc_off_4": dict(crc=ctypes.c_void_p(4096 + 2))}
CRC_UNSUPPORTED = {"B65536": dict(B=65536), "max_len_2GiB": dict(max_len=1 << 31, stride=1 << 31), "max_len_huge": dict(max_len=1 << 40, stride=1 << 40)}
WORKSPACE = {"null_ws": dict(ws=None), "short_ws": dict(wsb=255), "misaligned_ws": dict(ws=ctypes.c_void_p(4096 + 128)), "zero_ws": dict(wsb=0)}


def test_crc32_refusals():
    for name, kw in CRC_INVALID.items():
        assert crc_call(**kw) == _lib.E_INVALID, name
    for name, kw in CRC_UNSUPPORTED.items():
        assert crc_call(**kw) == _lib.E_UNSUPPORTED, name
    for name, kw in WORKSPACE.items():
        assert crc_call(**kw) == _lib.E_WORKSPACE, name
    assert crc_call(B=65536, max_len=0) == _lib.E_INVALID       # invalid wins over unsupported
    assert crc_call(B=65536, ws=None) == _lib.E_UNSUPPORTED     # and unsupported over the workspace
    assert crc_call(max_len=1 << 31, stride=1 << 31, wsb=0) == _lib.E_UNSUPPORTED
    need = _lib.load().srx_crc32_scratch_bytes(1, 100)
    assert crc_call(wsb=need - 1) == _lib.E_WORKSPACE
    # a short stride is one item's business only; NULL lengths are "every item is max_len long": both get as far as the workspace check
    assert crc_call(B=1, stride=0, wsb=0) == _lib.E_WORKSPACE
    assert crc_call(lengths=None, wsb=0) == _lib.E_WORKSPACE
    # the largest supported length passes the size check
    assert crc_call(max_len=(1 << 31) - 1, stride=(1 << 31) - 1, wsb=256) == _lib.E_WORKSPACE


def test_crc32_scratch_query():
    lib = _lib.load()
    for n in (1, SPAN, SEGMENT, SEGMENT + 1, 300001, (1 << 31) - 1):
        for b in (1, 3, 65535):
            s = lib.srx_crc32_scratch_bytes(b, n)
            assert s > 0 and s % 256 == 0 and s >= 4 * b * -(-n // SEGMENT)
        assert lib.srx_crc32_scratch_bytes(3, n) >= lib.srx_crc32_scratch_bytes(1, n)
    for b, n in ((0, 100), (-1, 100), (1, 0), (65536, 100), (1, 1 << 31), (1, 1 << 40)):
        assert lib.srx_crc32_scratch_bytes(b, n) == 0, (b, n)


FILE_ENTRIES = ("srx_png_file_u8", "srx_png_file_f32", "srx_png_file_f64")
FILE_OK = dict(img=FAKE, B=1, H=4, W=6, files=FAKE, lengths=FAKE, ws=FAKE, wsb=1 << 20)


def file_call(entry, **kw):
    a = dict(FILE_OK, **kw)
    return getattr(_lib.load(), entry)(a["img"], a["B"], a["H"], a["W"], a["files"], a["lengths"], a["ws"], a["wsb"], None)


FILE_INVALID = {"null_img": dict(img=None), "null_files": dict(files=None), "null_lengths": dict(lengths=None), "B0": dict(B=0), "B_neg": dict(B=-1),
                "H0": dict(H=0), "H_neg": dict(H=-4), "W0": dict(W=0), "W_neg": dict(W=-6)}
FILE_UNSUPPORTED = {"B65536": dict(B=65536), "raw_2GiB": dict(H=1 << 15, W=(1 << 16) - 1), "raw_over_int": dict(H=1 << 16, W=1 << 16),
                    "raw_2GiB_by_filter_bytes": dict(H=1 << 16, W=(1 << 15) - 1)}


@pytest.mark.parametrize("entry", FILE_ENTRIES)
def test_png_file_refusals(entry):
    for name, kw in FILE_INVALID.items():
        assert file_call(entry, **kw) == _lib.E_INVALID, name
    for name, kw in FILE_UNSUPPORTED.items():
        assert file_call(entry, **kw) == _lib.E_UNSUPPORTED, name
    for name, kw in WORKSPACE.items():
        assert file_call(entry, **kw) == _lib.E_WORKSPACE, name
    assert file_call(entry, B=65536, H=0) == _lib.E_INVALID          # invalid wins over unsupported
    assert file_call(entry, B=65536, ws=None) == _lib.E_UNSUPPORTED  # and unsupported over the workspace
    need = _lib.load().srx_png_file_scratch_bytes(1, 4, 6)
    assert file_call(entry, wsb=need - 1) == _lib.E_WORKSPACE


def test_the_largest_supported_image_passes_the_size_check():
    """H (W + 1) = 2^31 - 32768 is no refusal by size: with a short workspace the call gets as far as SRX_E_WORKSPACE"""
    for entry in FILE_ENTRIES:
        assert file_call(entry, H=(1 << 16) - 1, W=(1 << 15) - 1, wsb=256) == _lib.E_WORKSPACE


def test_png_file_queries():
    lib = _lib.load()
    for h, w in ((1, 1), (3, 5), (70, 1000), (2, 32767), (2, 32766), (97, 701), (3072, 4096), (1, 32767), (1, 32768)):
        assert lib.srx_png_file_bound(h, w) == PC.bound(h, w) + 57 == lib.srx_png_stream_bound(h, w) + 57, (h, w)
        for b in (1, 3, 65535):
            s = lib.srx_png_file_scratch_bytes(b, h, w)
            assert s > 0 and s % 256 == 0 and s >= lib.srx_png_scratch_bytes(b, h, w)
        assert lib.srx_png_file_scratch_bytes(3, h, w) >= lib.srx_png_file_scratch_bytes(1, h, w)
    for b, h, w in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (65536, 4, 4), (1, 1 << 15, (1 << 16) - 1), (1, 1 << 16, 1 << 16)):
        assert lib.srx_png_file_scratch_bytes(b, h, w) == 0, (b, h, w)
    assert lib.srx_png_file_bound(0, 5) == 0 and lib.srx_png_file_bound(5, -1) == 0


def test_names_are_in_the_header_the_ctypes_table_and_the_package():
    names = set(FILE_ENTRIES) | {"srx_crc32", "srx_crc32_scratch_bytes", "srx_png_file_bound", "srx_png_file_scratch_bytes"}
    assert names <= set(_lib.symbols())
    header = open(os.path.join(ROOT, "include", "srx.h")).read()
    for n in names:
        assert n + "(" in header, n
    for n in ("crc32", "png_file", "png_encode"):
        assert n in sr_mi355x.__all__, n
