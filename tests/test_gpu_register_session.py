"""Session driver with registration on the GPU (session.process_session(register=True), run_sr --register): a synthetic
mono_cal_target session (center.png, shift_0..3.png) and a two-rep barcode session are written to tmp_path with frames whose true
shifts are the nominal table plus a jitter; registration.json must carry estimates close to the truth, and a plain run must write
exactly the files and bytes it always did."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

from oracle import sr_oracle as O  # noqa: E402
from sr_mi355x import run_sr, session, synth  # noqa: E402

BOUND = 0.05  # LR px (the x2 estimates are ~0.015 off on these scenes; uint8 frames)


def frames_u8(truth, shifts, seed=1):
    lr = np.stack([O.forward_model(truth, synth.gaussian_psf(), s, 2) for s in shifts])
    lr = lr + np.random.default_rng(seed).normal(0.0, 1.0, lr.shape)
    return np.clip(np.rint(lr), 0, 255).astype(np.uint8)


def jittered(table, seed):
    t = np.asarray(table, dtype=np.float64)
    j = np.random.default_rng(seed).uniform(-0.15, 0.15, t.shape)
    return t + j


def files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_mono_cal_register_and_plain_run(tmp_path):
    table = [s for _, s in session.IMAGE_SHIFTS]
    true = jittered(table, 3)
    true[0] = 0.0  # the centre frame is the anchor: its table shift is its true one
    sess = tmp_path / "data" / "cal_target_synth"
    sess.mkdir(parents=True)
    for (fname, _), fr in zip(session.IMAGE_SHIFTS, frames_u8(synth.truth_image(320, 384, seed=2), true)):
        Image.fromarray(fr).save(sess / fname)
    common = ["--kind", "mono_cal_target", "--data-dir", str(tmp_path / "data")]
    run_sr.main(common + ["--output-dir", str(tmp_path / "reg"), "--register"])
    run_sr.main(common + ["--output-dir", str(tmp_path / "plain")])
    reg_dir, plain_dir = tmp_path / "reg" / "cal_target_synth", tmp_path / "plain" / "cal_target_synth"
    rep = json.load(open(reg_dir / "registration.json"))
    assert set(rep) == {"nominal", "estimated", "used", "score", "status"}
    assert np.array_equal(rep["nominal"], table)
    est, used = np.asarray(rep["estimated"]), np.asarray(rep["used"])
    assert rep["status"] == [0] * 5 and np.array_equal(est, used)
    assert np.array_equal(est[0], [0.0, 0.0])
    assert np.abs(est - true).max() < BOUND, (est, true)
    assert all(s > 0.95 for s in rep["score"])
    # a plain run: no registration.json, and the files a direct process_session call writes, to the byte
    assert "registration.json" not in os.listdir(plain_dir)
    session.process_session(str(sess), np.asarray(run_sr.api.make_gaussian_psf(session.PSF_SIZE, session.PSF_SIGMA)), str(tmp_path / "direct"),
                            verbose=False)
    assert files(plain_dir) == files(tmp_path / "direct" / "cal_target_synth")
    # the registered reconstruction used other shifts
    assert files(reg_dir)["SAA.png"] != files(plain_dir)["SAA.png"]
    assert set(files(reg_dir)) == set(files(plain_dir)) | {"registration.json"}


def test_barcode_reps_register_one_item_per_rep(tmp_path):
    table = session.CORNER_SHIFTS
    sess = tmp_path / "data" / "barcodes"
    sess.mkdir(parents=True)
    truths = []
    for rep in range(2):
        true = jittered(table, 10 + rep)
        truths.append(true)
        for c, fr in enumerate(frames_u8(synth.truth_image(256, 288, seed=5 + rep), true, seed=rep)):
            Image.fromarray(fr).save(sess / f"corner{c}_rep{rep:02d}.png")
    psf = synth.gaussian_psf()
    written = session.process_session(str(sess), psf, str(tmp_path / "reg"), kind="mono_barcodes", n_iter=3, verbose=False, register=True)
    assert [os.path.basename(w) for w in written] == ["rep0", "rep1"]
    for d, true in zip(written, truths):
        rep = json.load(open(os.path.join(d, "registration.json")))
        est = np.asarray(rep["estimated"])
        assert rep["status"] == [0] * 4
        # anchored at the table's corner 0: differences to frame 0 carry the truth
        assert np.array_equal(est[0], table[0])
        assert np.abs((est - est[0]) - (true - true[0])).max() < BOUND, (est, true)
    plain = session.process_session(str(sess), psf, str(tmp_path / "plain"), kind="mono_barcodes", n_iter=3, verbose=False)
    for d in plain:
        assert "registration.json" not in os.listdir(d)
