"""Inputs, references and comparisons shared by tests/test_edge_sfr_host.py and tests/test_gpu_edge_sfr.py (a plain helper module like
png_cases.py: no fixtures, nothing registered).

  rois()            the two 200 x 200 ROIs of tests/golden/metrics.npz and eight seeded noisy synthetic edges (40 x 40, 37 x 53, 48 x 64, 64 x 48
                    at 0.3 / 0.35 / 1.2 / 1.25 rad), all uint8: integer samples, so every sum of the device form is exact
  reference()       sr_mi355x.metrics on a ROI, step for step, with the intermediate values srx_edge_sfr_* reports (threshold, counts)
  build_model()     tests/edge_sfr_host_model.cpp (the plain arithmetic of csrc/srx_sfr.hpp) compiled with g++; run_model() runs it on a ROI
  close_to_reference / same_bits   the two comparisons: the tolerances tests/test_gpu_metrics.py holds the device composition to, and bit identity
"""
import os
import shutil
import subprocess

import numpy as np

from sr_mi355x import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "enph459-super-resolution_amd", "csrc")
GXX = shutil.which("g++")
MAX_BINS, SUMMARY = 80, 16
HR_PITCH = M.SENSOR_PITCH_MM / 2
FIELDS = ("mtf50", "mtf10", "angle_deg", "m", "b", "rows_are_x", "threshold", "n_edge", "n_side", "nbin", "lo", "hi", "flipped", "m_c", "b_c", "zero")
SIDES = {"left": 0, "right": 1}
SYNTH = [(40, 40, 0.3), (37, 53, 0.35), (48, 64, 1.2), (64, 48, 1.25), (40, 40, 1.2), (37, 53, 1.25), (48, 64, 0.3), (64, 48, 0.35)]


def edge(h, w, angle, seed, width=0.9, noise=1.5, offset=0.0):
    """a soft edge through the centre of an h x w ROI, its normal at `angle` to the x axis, with seeded Gaussian noise; float64 in 0..255"""
    yy, xx = np.mgrid[0:h, 0:w]
    d = (xx - 0.5 * (w - 1)) * np.cos(angle) + (yy - 0.5 * (h - 1)) * np.sin(angle) - offset
    img = 40.0 + 170.0 / (1.0 + np.exp(-d / width))
    return np.clip(img + np.random.default_rng(seed).normal(0.0, noise, img.shape), 0, 255)


def rois():
    g = np.load(os.path.join(ROOT, "tests", "golden", "metrics.npz"))
    out = {"golden_native_2x": np.ascontiguousarray(g["native_2x_roi"]), "golden_SAA": np.ascontiguousarray(g["SAA_roi"])}
    for k, (h, w, a) in enumerate(SYNTH):
        out[f"synth_{h}x{w}_{a}"] = edge(h, w, a, seed=100 + k).astype(np.uint8)
    return out


def zero_plane(n=256):
    """constant outside |d| < 7 of a noisy edge: more than 85 % of the Sobel magnitudes are exactly 0, so the threshold is 0.0 between tied
    order statistics and every pixel with a nonzero magnitude is an edge pixel"""
    yy, xx = np.mgrid[0:n, 0:n]
    d = (xx - 0.5 * (n - 1)) * np.cos(0.35) + (yy - 0.5 * (n - 1)) * np.sin(0.35)
    img = edge(n, n, 0.35, seed=77)
    img[d <= -7] = 40.0
    img[d >= 7] = 210.0
    return img.astype(np.uint8)


def step(h, w, seed, axis=1):
    """a noisy step across the middle of a thin h x w ROI (axis 1: between two columns), uint8"""
    a = np.full((h, w), 40.0)
    if axis == 1:
        a[:, w // 2:] = 210.0
    else:
        a[h // 2:, :] = 210.0
    return np.clip(a + np.random.default_rng(seed).normal(0.0, 1.5, a.shape), 0, 255).astype(np.uint8)


def status_cases():
    """name -> (uint8 ROI, the status of both sides).  One row: every edge pixel lies ON the centre line, none on a side (2).  Two rows or
    two columns: the side's pixels share one v, the distances are 0 and 1, four bins of which one is filled (4, found by k_sfr_tail after
    k_sfr_bins ran).  Three rows and 12 x 12: status 0 with 12 / 13 and 53 bins, the outputs zero behind them."""
    return {"one_row_1x200": (step(1, 200, 1), 2), "two_rows_2x200": (step(2, 200, 2), 4), "two_columns_200x2": (step(200, 2, 4, axis=0), 4),
            "three_rows_3x200": (step(3, 200, 3), 0), "small_12x12": (edge(12, 12, 0.3, seed=1).astype(np.uint8), 0)}


def same_failed_item(dev, model):
    """a nonzero status: the same status, the summary's fields the same bits (NaN where not reached) except the angle (atan2: 1e-9, or NaN
    on both sides), esf and mtf NaN throughout"""
    assert dev["status"] == model["status"] != 0
    for k in FIELDS:
        if k != "angle_deg":
            assert (np.isnan(dev[k]) and np.isnan(model[k])) or bits(dev[k]) == bits(model[k]), (k, dev[k], model[k])
    assert (np.isnan(dev["angle_deg"]) and np.isnan(model["angle_deg"])) or abs(dev["angle_deg"] - model["angle_deg"]) <= 1e-9
    assert np.isnan(dev["esf"]).all() and np.isnan(dev["mtf_raw"]).all() and dev["zero"] == 0.0


def magnitude(roi):
    smooth = M._gaussian_filter(np.asarray(roi).astype(np.float64), 1.5)
    return np.sqrt(M._sobel(smooth, 1) ** 2 + M._sobel(smooth, 0) ** 2)


_REF = {}


def reference(roi, side, key=None):
    """metrics.slanted_edge_esf -> esf_to_mtf -> mtf_at_fraction on `roi`, plus the intermediate values of slanted_edge_esf (recomputed with
    its own expressions); computed once per `key`"""
    if key is not None and (key, side) in _REF:
        return _REF[key, side]
    roi = np.asarray(roi)
    mag = magnitude(roi)
    thr = np.percentile(mag, 85)
    rs, cs = np.where(mag > thr)
    rows_are_x = bool((rs.max() - rs.min()) >= (cs.max() - cs.min()))
    u, v = (rs, cs) if rows_are_x else (cs, rs)
    m_c, b_c = np.polyfit(u, v, 1)
    dist = (v - m_c * u - b_c) / np.sqrt(1 + m_c ** 2)
    sel = dist < 0 if side == "left" else dist > 0
    m, b = np.polyfit(u[sel], v[sel], 1)
    ex, ey, ang = M.slanted_edge_esf(roi, side=side)
    fr, mtf, _ = M.esf_to_mtf(ex, ey)
    fc = fr / HR_PITCH
    pos = fc > 0
    ref = dict(threshold=float(thr), n_edge=len(rs), n_side=int(sel.sum()), rows_are_x=rows_are_x, nbin=len(ex), m=float(m), b=float(b), m_c=float(m_c),
               b_c=float(b_c), esf_x=ex, esf_y=ey, angle_deg=float(ang), freq=fr, mtf=mtf,
               mtf50_mm=float(M.mtf_at_fraction(fc[pos], mtf[pos], 0.5)), mtf10_mm=float(M.mtf_at_fraction(fc[pos], mtf[pos], 0.1)))
    if key is not None:
        _REF[key, side] = ref
    return ref


def item(status, summary, esf, mtf):
    """one item's outputs as the dict the comparisons take (what metrics_device.edge_sfr(...).result() returns per item)"""
    summary, esf, mtf = np.asarray(summary, np.float64), np.asarray(esf, np.float64).reshape(2, MAX_BINS), np.asarray(mtf, np.float64).reshape(2, MAX_BINS // 2)
    d = dict(zip(FIELDS, (float(x) for x in summary)))
    nbin = int(d["nbin"]) if status == 0 else 0
    d.update(status=int(status), summary=summary, esf=esf, mtf_raw=mtf, esf_x=esf[0, :nbin], esf_y=esf[1, :nbin], freq=mtf[0, :nbin // 2],
             mtf=mtf[1, :nbin // 2])
    return d


def close_to_reference(got, ref, exact_threshold=True):
    """the issue's bounds: threshold and counts equal, esf_x and angle 1e-9, esf_y and mtf 1e-8, MTF50 / MTF10 in cycles/mm 1e-6"""
    assert got["status"] == 0
    if exact_threshold:
        assert got["threshold"] == ref["threshold"]
    for k in ("n_edge", "n_side", "rows_are_x", "nbin"):
        assert got[k] == ref[k], (k, got[k], ref[k])
    np.testing.assert_allclose(got["esf_x"], ref["esf_x"], rtol=0, atol=1e-9)
    assert abs(got["angle_deg"] - ref["angle_deg"]) <= 1e-9
    np.testing.assert_allclose(got["esf_y"], ref["esf_y"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(got["mtf"], ref["mtf"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(got["freq"], ref["freq"], rtol=0, atol=1e-9)
    assert np.isfinite(ref["mtf50_mm"]) and np.isfinite(ref["mtf10_mm"])
    assert abs(got["mtf50"] / HR_PITCH - ref["mtf50_mm"]) <= 1e-6 and abs(got["mtf10"] / HR_PITCH - ref["mtf10_mm"]) <= 1e-6
    nbin = int(got["nbin"])
    assert (got["esf"][:, nbin:] == 0).all() and (got["mtf_raw"][:, nbin // 2:] == 0).all() and got["zero"] == 0.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same_integer_part(dev, model):
    """device against the host model on integer samples: everything up to the ESF is the same bits (all sums are integers); the
    trigonometric tail is held to the reference's tolerances"""
    assert dev["status"] == model["status"] == 0
    for k in ("threshold", "n_edge", "n_side", "rows_are_x", "m_c", "b_c", "m", "b", "lo", "hi", "nbin", "flipped", "zero"):
        assert bits(dev[k]) == bits(model[k]), (k, dev[k], model[k])
    assert np.array_equal(bits(dev["esf"]), bits(model["esf"]))
    np.testing.assert_allclose(dev["mtf_raw"], model["mtf_raw"], rtol=0, atol=1e-8)
    assert abs(dev["angle_deg"] - model["angle_deg"]) <= 1e-9
    for k in ("mtf50", "mtf10"):  # (a curve that never falls through: NaN on both sides)
        assert (np.isnan(dev[k]) and np.isnan(model[k])) or abs(dev[k] - model[k]) / HR_PITCH <= 1e-6, (k, dev[k], model[k])


def build_model(path, sanitize=True):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([GXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-I" + CSRC, "-o", path,
                                                                                                     os.path.join(ROOT, "tests", "edge_sfr_host_model.cpp")])
    return path


def _run(args):
    r = subprocess.run(args, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f"exit {r.returncode}\n{r.stderr[-3000:]}"
    return r.stdout


def run_model(exe, tmp, roi, side, sigma=1.5):
    roi = np.asarray(roi)
    src = os.path.join(str(tmp), "roi.bin")
    with open(src, "wb") as fp:
        fp.write(np.asarray(roi.shape, np.int32).tobytes() + np.ascontiguousarray(roi, dtype=np.float64).tobytes())
    lines = {ln.split()[0]: ln.split()[1:] for ln in _run([exe, "sfr", src, str(SIDES[side]), repr(float(sigma))]).splitlines()}
    return item(int(lines["status"][0]), [float(x) for x in lines["summary"]], [float(x) for x in lines["esf"]], [float(x) for x in lines["mtf"]])


def model_percentile(exe, tmp, a):
    src = os.path.join(str(tmp), "values.bin")
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    with open(src, "wb") as fp:
        fp.write(np.asarray([a.size], np.int64).tobytes() + a.tobytes())
    return float(_run([exe, "percentile", src]))
