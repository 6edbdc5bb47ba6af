"""Pins the oracle to the result PNGs the reference COMMITTED: a fresh
oracle run on the reference's committed full-size inputs must reproduce native_2x.png /
SAA.png / LR_(red_)mean.png (uint8, truncating quantiser).  "Reproduce" = identical pixel
for pixel, except truncation knife-edges: the charts have large flat areas where the exact
result is a whole number (e.g. 255.0), SciPy's and the oracle's float64 round-off land on
either side of it (|delta| ~ 1e-13) and `astype(uint8)` truncates them to v and v-1.  So a
differing pixel is accepted only if it is off by exactly 1 LSB AND the oracle's float64
value is within 1e-9 of that whole number.  Needs a checkout of the reference repository, named
by SR_REFERENCE (its full-size frames and results are too large for tests/golden/; the same
functions are pinned on crops of them by test_oracle_golden.py::test_real_crops); skipped
without one.  The committed SAA_IBP.png files are stale (older script version) and are NOT used."""
import glob
import json
import os

import numpy as np
import pytest
from PIL import Image

from oracle import sr_oracle as O

REF = os.environ.get("SR_REFERENCE", "")
pytestmark = pytest.mark.skipif(not (REF and os.path.isdir(os.path.join(REF, "rgb_cal_target"))),
                                reason="needs a checkout of the reference repository: set SR_REFERENCE to it")


def png(path):
    return np.array(Image.open(path))


def same_image(x64, committed):
    q = O.quantize_u8(x64).astype(np.int16)
    ref = committed.astype(np.int16)
    diff = q != ref
    if not diff.any():
        return True
    assert np.abs(q - ref)[diff].max() == 1
    xv = x64[diff]
    assert np.abs(xv - np.rint(xv)).max() < 1e-9, "a non-knife-edge pixel differs"
    return True


def test_rgb_cal_target_committed():
    O.set_threads(8)
    try:
        combo = glob.glob(os.path.join(REF, "rgb_cal_target", "data", "*"))[0]
        res = glob.glob(os.path.join(REF, "rgb_cal_target", "results", "*"))[0]
        meta = json.load(open(os.path.join(combo, "metadata.json")))
        labels = ['(-x,+y)', '(+x,+y)', '(-x,-y)', '(+x,-y)']           # rgb_cal_target/run_sr.py:63
        shifts = [(meta["expected_shifts"][l]["dy_px"] / 2.0, meta["expected_shifts"][l]["dx_px"] / 2.0)
                  for l in labels]                                         # :88-92
        assert json.load(open(os.path.join(res, "shifts.json")))["shifts_lr_yx"] == [list(s) for s in shifts]
        frames = []
        for idx in range(4):
            reps = sorted(glob.glob(os.path.join(combo, f"corner{idx}_rep*.png")))
            frames.append(O.mean0(np.stack([O.extract_red(png(r).astype(np.float64)) for r in reps])))
        mean_lr = O.mean0(np.stack(frames))
        assert np.array_equal(O.quantize_u8(mean_lr), png(os.path.join(res, "LR_red_mean.png")))
        assert same_image(O.ndi_zoom(mean_lr, 2), png(os.path.join(res, "native_2x.png")))
        saa = O.shift_and_add(frames, shifts, 2)
        assert same_image(saa, png(os.path.join(res, "SAA.png")))
    finally:
        O.set_threads(1)


def test_mono_cal_target_committed():
    O.set_threads(8)
    try:
        sess = glob.glob(os.path.join(REF, "mono_cal_target", "data", "*"))[0]
        res = glob.glob(os.path.join(REF, "mono_cal_target", "results", "*"))[0]
        names = ["center.png", "shift_0.png", "shift_1.png", "shift_2.png", "shift_3.png"]   # :59-66
        shifts = [(0.0, 0.0), (0.5, -0.5), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)]
        frames = [png(os.path.join(sess, n)).astype(np.float64) for n in names]
        mean_lr = O.mean0(np.stack(frames))
        assert np.array_equal(O.quantize_u8(mean_lr), png(os.path.join(res, "LR_mean.png")))
        assert same_image(O.ndi_zoom(mean_lr, 2), png(os.path.join(res, "native_2x.png")))
        saa = O.shift_and_add(frames, shifts, 2)
        assert same_image(saa, png(os.path.join(res, "SAA.png")))
    finally:
        O.set_threads(1)
