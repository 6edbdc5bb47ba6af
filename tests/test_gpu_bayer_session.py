"""The session driver with colour=True (run_sr --colour) on synthetic raw RGGB sessions: every file of the plain run is written byte for
byte, and beside them the three RGB PNGs -- whose red channel holds the grey file's pixels -- and convergence_planes.json."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from sr_mi355x import session, synth

pytestmark = pytest.mark.gpu
H, W, N_ITER = 64, 96, 3
REG_H, REG_W = 96, 112   # registration needs planes of at least 40 x 40 (a 12-pixel margin around a 16 x 16 crop)
GREY = ("native_2x.png", "SAA.png", "SAA_IBP.png")


def raw_frame(k, seed, H=H, W=W):
    """a smooth coloured scene, shifted a little from frame to frame, through an RGGB mosaic, with noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    scene = 110 + 70 * np.sin(0.19 * (xx + 0.5 * k)) * np.cos(0.23 * (yy - 0.5 * k))
    scene[0::2, 0::2] *= 1.25
    scene[1::2, 1::2] *= 0.6
    return np.clip(np.rint(scene + rng.normal(0, 2, (H, W))), 0, 255).astype(np.uint8)


def write_sessions(root, H, W):
    bc = root / "barcodes"
    bc.mkdir()
    for rep in range(2):
        for c in range(4):
            session.write_png_u8(str(bc / f"corner{c}_rep{rep:02d}.png"), raw_frame(c, 10 * rep + c, H, W))
    combo = root / "combo"
    combo.mkdir()
    for c in range(4):
        for rep in range(3):
            session.write_png_u8(str(combo / f"corner{c}_rep{rep:02d}.png"), raw_frame(c, 100 + 10 * rep + c, H, W))
    meta = {"expected_shifts": {lab: {"dy_px": 2.0 * s[0], "dx_px": 2.0 * s[1]} for lab, s in zip(session.CORNER_ORDER, session.CORNER_SHIFTS)}}
    (combo / "metadata.json").write_text(json.dumps(meta))
    return {"rgb_barcodes": str(bc), "rgb_cal_target": str(combo), "size": (H, W)}


@pytest.fixture(scope="module")
def sessions(tmp_path_factory):
    return write_sessions(tmp_path_factory.mktemp("bayer_sessions"), H, W)


@pytest.fixture(scope="module")
def sessions_reg(tmp_path_factory):
    return write_sessions(tmp_path_factory.mktemp("bayer_sessions_reg"), REG_H, REG_W)


def files_of(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


@pytest.mark.parametrize("mode", [dict(), dict(keep_u8=True, device_png=True), dict(register=True)], ids=["plain", "u8_devpng", "register"])
@pytest.mark.parametrize("kind", ["rgb_barcodes", "rgb_cal_target"])
def test_colour_adds_files_and_changes_none(tmp_path, sessions, sessions_reg, kind, mode):
    psf = synth.gaussian_psf()
    sessions = sessions_reg if mode.get("register") else sessions
    H, W = sessions["size"]
    plain = session.process_session(sessions[kind], psf, str(tmp_path / "plain"), kind=kind, n_iter=N_ITER, verbose=False, **mode)
    colour = session.process_session(sessions[kind], psf, str(tmp_path / "colour"), kind=kind, n_iter=N_ITER, verbose=False, colour=True, **mode)
    assert len(plain) == len(colour) == (2 if kind == "rgb_barcodes" else 1)
    for a, b in zip(plain, colour):
        fa, fb = files_of(a), files_of(b)
        assert "done.flag" in fa and len(fa) >= 6
        for name, data in fa.items():
            assert fb[name] == data, f"{name} differs with colour=True"
        assert ("registration.json" in fa) == bool(mode.get("register"))
        assert set(fb) - set(fa) == {"native_2x_rgb.png", "SAA_rgb.png", "SAA_IBP_rgb.png", "convergence_planes.json"}
        for name in GREY:
            im = Image.open(os.path.join(b, name[:-4] + "_rgb.png"))
            assert im.mode == "RGB" and im.size == (W, H)   # planes of (H / 2, W / 2) at factor 2
            assert np.array_equal(np.asarray(im)[..., 0], np.asarray(Image.open(os.path.join(b, name)))), name
        planes = json.load(open(os.path.join(b, "convergence_planes.json")))["ibp_mse"]
        assert len(planes) == 4 and all(len(t) == N_ITER for t in planes)
        assert planes[0] == json.load(open(os.path.join(b, "convergence.json")))["ibp_mse"]
    assert session.process_session(sessions[kind], psf, str(tmp_path / "colour"), kind=kind, n_iter=N_ITER, verbose=False, colour=True, **mode) == []


def test_device_and_host_rgb_files_hold_the_same_pixels(tmp_path, sessions):
    psf = synth.gaussian_psf()
    kind = "rgb_cal_target"
    host = session.process_session(sessions[kind], psf, str(tmp_path / "host"), kind=kind, n_iter=N_ITER, verbose=False, colour=True)[0]
    dev = session.process_session(sessions[kind], psf, str(tmp_path / "dev"), kind=kind, n_iter=N_ITER, verbose=False, colour=True, device_png=True)[0]
    for name in GREY:
        rgb = name[:-4] + "_rgb.png"
        assert np.array_equal(np.asarray(Image.open(os.path.join(host, rgb))), np.asarray(Image.open(os.path.join(dev, rgb)))), rgb


def test_colour_is_refused_where_it_does_not_apply(tmp_path, sessions):
    psf = synth.gaussian_psf()
    with pytest.raises(ValueError, match="rgb_"):
        session.process_session(sessions["rgb_barcodes"], psf, str(tmp_path / "x"), kind="mono_barcodes", verbose=False, colour=True)
    with pytest.raises(ValueError, match="patchwise"):
        session.process_session(sessions["rgb_cal_target"], psf, str(tmp_path / "x"), kind="rgb_cal_target", verbose=False, colour=True, patchwise="global")
    with pytest.raises(ValueError, match="row_bands"):
        session.process_session(sessions["rgb_cal_target"], psf, str(tmp_path / "x"), kind="rgb_cal_target", verbose=False, colour=True, row_bands=True)
    assert not os.path.exists(tmp_path / "x")


def test_loaders_default_is_the_red_plane_of_all(sessions):
    for keep in (False, True):
        red, shifts = session.load_rgb_cal_combo(sessions["rgb_cal_target"], keep_u8=keep)
        every, shifts_all = session.load_rgb_cal_combo(sessions["rgb_cal_target"], keep_u8=keep, planes="all")
        assert shifts == shifts_all and len(red) == len(every) == 4
        for a, b in zip(red, every):
            assert tuple(b.shape) == (4, H // 2, W // 2) and torch.equal(a, b[0])
        reps, _ = session.load_corner_reps(sessions["rgb_barcodes"], True, keep_u8=keep)
        reps_all, _ = session.load_corner_reps(sessions["rgb_barcodes"], "all", keep_u8=keep)
        assert len(reps) == len(reps_all) == 2
        for fr, fr_all in zip(reps, reps_all):
            for a, b in zip(fr, fr_all):
                assert b.dtype == (torch.uint8 if keep else torch.float64) and tuple(b.shape) == (4, H // 2, W // 2) and torch.equal(a, b[0])


def test_the_multi_session_loop_writes_the_same_files(tmp_path, sessions):
    """process_sessions (the Prefetcher loads with colour=True ahead of the device work) against process_session, uint8 frames"""
    psf = synth.gaussian_psf()
    kind = "rgb_barcodes"
    one = session.process_session(sessions[kind], psf, str(tmp_path / "one"), kind=kind, n_iter=N_ITER, verbose=False, colour=True, keep_u8=True)
    many = session.process_sessions([sessions[kind]], psf, str(tmp_path / "many"), kind, n_iter=N_ITER, verbose=False, colour=True, keep_u8=True)
    assert len(one) == len(many) == 2
    for a, b in zip(one, many):
        assert files_of(a) == files_of(b) and "SAA_IBP_rgb.png" in files_of(b)
