"""The colour entry points' boundary without a GPU (include/srx_bayer.h): every declared name is exported and bound, srx.h and its census
(_lib.symbols()) know none of them, every refusal is decided on the host before any HIP call -- the pointers are never dereferenced --
in the documented order, the PNG queries are the grey ones at width 3 W, and the numpy merge model on a case small enough to write out."""
import ctypes
import os
import re

import numpy as np
import pytest

import bayer_cases as BC
from sr_mi355x import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = ctypes.c_void_p(4096)
GAINS = (ctypes.c_double * 3)(1.0, 1.0, 1.0)
INV, UNS, WSP = _lib.E_INVALID, _lib.E_UNSUPPORTED, _lib.E_WORKSPACE


def header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(srx_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    _lib.build()
    lib = _lib.load()
    hdr = header_symbols("srx_bayer.h")
    assert len(hdr) == 11
    for name in hdr:
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name} is exported but load() did not bind it"
    assert sorted(_lib.bayer_symbols()) == hdr, "the _BAYER table and include/srx_bayer.h disagree"


def test_srx_h_and_its_census_know_none_of_the_new_names():
    new = set(_lib.bayer_symbols())
    assert not new & set(header_symbols("srx.h"))
    assert not new & set(_lib.symbols())
    assert not [n for n in new if n.endswith("_workspace_bytes") or n.endswith("_workspace_bytes_for")]


# ---- refusals: (arguments that pass, {case: changes}) per entry point ----
def split(kind="u8", raw=FAKE, B=1, H=4, W=6, out=FAKE):
    return getattr(_lib.load(), "srx_bayer_split_" + kind)(raw, B, H, W, out, None)


def mean(raw=FAKE, B=1, R=2, H=4, W=6, eb=4, out=FAKE):
    return _lib.load().srx_bayer_mean_u8(raw, B, R, H, W, eb, out, None)


def merge(entry="srx_bayer_merge", kind="f32", planes=FAKE, B=1, Hp=4, Wp=6, d=1, gains=GAINS, out=FAKE):
    return getattr(_lib.load(), f"{entry}_{kind}")(planes, B, Hp, Wp, d, gains, out, None)


def png(img=FAKE, B=1, H=4, W=6, files=FAKE, lengths=FAKE, ws=FAKE, wsb=1 << 20):
    return _lib.load().srx_png_file_rgb8(img, B, H, W, files, lengths, ws, wsb, None)


SIZES_INVALID = {"B0": dict(B=0), "B_neg": dict(B=-1), "H0": dict(H=0), "H_neg": dict(H=-4), "W0": dict(W=0), "W_neg": dict(W=-6)}
SPLIT_INVALID = dict(SIZES_INVALID, null_raw=dict(raw=None), null_planes=dict(out=None))
SPLIT_UNSUPPORTED = {"H_odd": dict(H=5), "W_odd": dict(W=7), "B65536": dict(B=65536)}
SPLIT_2GIB = {"u8": dict(H=1 << 15, W=1 << 16), "f32": dict(H=1 << 15, W=1 << 14), "f64": dict(H=1 << 14, W=1 << 14)}   # exactly 2 GiB each


@pytest.mark.parametrize("kind", ["u8", "f32", "f64"])
def test_split_refusals(kind):
    for case, kw in SPLIT_INVALID.items():
        assert split(kind, **kw) == INV, case
    for case, kw in dict(SPLIT_UNSUPPORTED, item_2GiB=SPLIT_2GIB[kind]).items():
        assert split(kind, **kw) == UNS, case
    assert split(kind, H=5, B=0) == INV and split(kind, B=65536, out=None) == INV   # invalid wins over unsupported


def test_mean_refusals():
    for case, kw in dict(SIZES_INVALID, null_raw=dict(raw=None), null_planes=dict(out=None), R0=dict(R=0), R_neg=dict(R=-3), eb0=dict(eb=0),
                         eb2=dict(eb=2), eb16=dict(eb=16)).items():
        assert mean(**kw) == INV, case
    for case, kw in {"H_odd": dict(H=5), "W_odd": dict(W=7), "R65536": dict(R=65536), "B65536": dict(B=65536),
                     "item_2GiB": dict(R=2, H=1 << 15, W=1 << 15), "item_2GiB_by_R": dict(R=32768, H=256, W=256),
                     "frame_over_int": dict(R=1, H=1 << 16, W=1 << 16)}.items():
        assert mean(**kw) == UNS, case
    assert mean(W=7, eb=2) == INV and mean(R=65536, B=0) == INV


@pytest.mark.parametrize("entry", ["srx_bayer_merge", "srx_bayer_merge_rgb8"])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_merge_refusals(entry, kind):
    for case, kw in {"null_planes": dict(planes=None), "null_out": dict(out=None), "B0": dict(B=0), "B_neg": dict(B=-2), "Hp0": dict(Hp=0),
                     "Hp_neg": dict(Hp=-1), "Wp0": dict(Wp=0), "Wp_neg": dict(Wp=-1), "d_neg": dict(d=-1)}.items():
        assert merge(entry, kind, **kw) == INV, case
    plane_2gib = dict(Hp=1 << 15, Wp=(1 << 14) if kind == "f32" else (1 << 13))
    for case, kw in {"plane_2GiB": plane_2gib, "B65536": dict(B=65536), "plane_over_int": dict(Hp=1 << 16, Wp=1 << 16)}.items():
        assert merge(entry, kind, **kw) == UNS, case
        assert merge(entry, kind, gains=None, **kw) == UNS, case
    assert merge(entry, kind, B=65536, d=-1) == INV


def test_png_refusals():
    for case, kw in dict(SIZES_INVALID, null_img=dict(img=None), null_files=dict(files=None), null_lengths=dict(lengths=None)).items():
        assert png(**kw) == INV, case
    for case, kw in {"3W_over_int": dict(W=(1 << 31) // 3 + 1), "B65536": dict(B=65536), "scanlines_2GiB": dict(H=1 << 16, W=1 << 14)}.items():
        assert png(**kw) == UNS, case
    lib = _lib.load()
    need = lib.srx_png_file_rgb8_scratch_bytes(1, 4, 6)
    assert need > 0
    for case, kw in {"null_ws": dict(ws=None, wsb=need), "short_ws": dict(wsb=need - 1), "misaligned_ws": dict(ws=ctypes.c_void_p(4096 + 64), wsb=need)}.items():
        assert png(**kw) == WSP, case
    assert png(B=65536, H=0) == INV and png(B=65536, ws=None) == UNS   # invalid, then unsupported, then the workspace


@pytest.mark.parametrize("H,W", BC.PNG_SHAPES + [(70, 1000), (1536, 2048)])
def test_png_queries_are_the_grey_ones_at_three_times_the_width(H, W):
    lib = _lib.load()
    assert lib.srx_png_file_rgb8_bound(H, W) == lib.srx_png_file_bound(H, 3 * W) > 0
    for B in (1, 2, 7):
        assert lib.srx_png_file_rgb8_scratch_bytes(B, H, W) == lib.srx_png_file_scratch_bytes(B, H, 3 * W) > 0


def test_png_queries_of_refused_shapes_are_zero():
    lib = _lib.load()
    assert lib.srx_png_file_rgb8_bound(0, 4) == 0 and lib.srx_png_file_rgb8_bound(4, -1) == 0
    assert lib.srx_png_file_rgb8_bound(4, (1 << 31) // 3 + 1) == 0
    assert lib.srx_png_file_rgb8_scratch_bytes(0, 4, 4) == 0 and lib.srx_png_file_rgb8_scratch_bytes(65536, 4, 4) == 0
    assert lib.srx_png_file_rgb8_scratch_bytes(1, 4, (1 << 31) // 3 + 1) == 0


def test_merge_model_by_hand():
    """2 x 2 planes, d = 1: G1 and B read one sample to the left, G2 and B one up, clamped"""
    P = np.array([[[[1, 2], [3, 4]], [[10, 20], [30, 40]], [[100, 200], [300, 400]], [[5, 6], [7, 8]]]], dtype=np.float64)
    rgb = BC.merge_model(P, 1, None, "f64")
    assert np.array_equal(rgb[0, 0], [[1, 2], [3, 4]])
    # g1 = P1[y, c(x - 1)] = [[10, 10], [30, 30]]; g2 = P2[c(y - 1), x] = [[100, 200], [100, 200]]
    assert np.array_equal(rgb[0, 1], [[55, 105], [65, 115]])
    # B = P3[c(y - 1), c(x - 1)]: every sample reads P3[0, 0], all but [1, 1] through a clamp
    assert np.array_equal(rgb[0, 2], [[5, 5], [5, 5]])
    assert np.array_equal(BC.merge_model(P, 0, None, "f64")[0, 2], P[0, 3])   # d = 0 stacks the planes
    g = BC.merge_model(P, 1, (1.5, 1.0, 0.75), "f32")
    assert g.dtype == np.float32 and np.array_equal(g[0, 0], [[1.5, 3], [4.5, 6]]) and np.array_equal(g[0, 2], np.full((2, 2), 3.75))
    q = BC.rgb8_model(P, 1, (1.5, 1.0, 0.75), "f32")
    assert q.shape == (1, 2, 2, 3) and q.dtype == np.uint8 and list(q[0, 1, 1]) == [6, 115, 3]


def test_split_and_mean_models():
    raw = np.arange(2 * 4 * 6, dtype=np.uint8).reshape(2, 4, 6)
    pl = BC.split_model(raw)
    assert pl.shape == (2, 4, 2, 3)
    assert np.array_equal(pl[1, 0], raw[1, 0::2, 0::2]) and np.array_equal(pl[1, 1], raw[1, 0::2, 1::2])
    assert np.array_equal(pl[1, 2], raw[1, 1::2, 0::2]) and np.array_equal(pl[1, 3], raw[1, 1::2, 1::2])
    m = BC.mean_model(raw[None], "f32")
    assert m.dtype == np.float32 and np.array_equal(m[0], BC.split_model((raw[0].astype(np.float32) + raw[1]) / np.float32(2)))


@pytest.mark.parametrize("argv,why", [(["--kind", "mono_barcodes"], "rgb_"), (["--kind", "mono_cal_target"], "rgb_"),
                                      (["--kind", "rgb_cal_target", "--patchwise", "global"], "patchwise"),
                                      (["--kind", "rgb_cal_target", "--row-bands"], "row-bands")])
def test_run_sr_refuses_colour_where_it_does_not_apply(argv, why, tmp_path, capsys):
    from sr_mi355x import run_sr
    with pytest.raises(SystemExit) as e:
        run_sr.main(argv + ["--colour", "--data-dir", str(tmp_path), "--output-dir", str(tmp_path / "out")])
    assert e.value.code == 2 and "--colour" in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


def test_process_sessions_refuses_colour_before_any_work(tmp_path):
    from sr_mi355x import session
    for kw, kind in ((dict(), "mono_barcodes"), (dict(patchwise="local"), "rgb_cal_target"), (dict(row_bands=True), "rgb_cal_target")):
        with pytest.raises(ValueError, match="colour"):
            session.process_sessions([str(tmp_path)], np.ones((7, 7)) / 49, str(tmp_path / "out"), kind, verbose=False, colour=True, **kw)
    assert not (tmp_path / "out").exists()


def test_host_rgb_writer_and_container(tmp_path):
    """write_png_rgb8: PIL reads the pixels back, and the grey container has not changed"""
    import io
    from PIL import Image
    from sr_mi355x import session
    img = np.random.default_rng(3).integers(0, 256, (5, 43, 3), dtype=np.uint8)
    session.write_png_rgb8(str(tmp_path / "a.png"), img)
    im = Image.open(str(tmp_path / "a.png"))
    assert im.mode == "RGB" and np.array_equal(np.asarray(im), img)
    data = open(tmp_path / "a.png", "rb").read()
    assert data[:33] == BC.rgb_container(43, 5, b"")[:33]   # signature + truecolour IHDR
    grey = session.png_container(43, 5, b"xyz")
    assert grey[25] == 0 and session.png_container(43, 5, b"xyz", colour_type=2)[25] == 2
    assert Image.open(io.BytesIO(data)).size == (43, 5)
    with pytest.raises(ValueError):
        session.write_png_rgb8(str(tmp_path / "b.png"), img[..., 0])
