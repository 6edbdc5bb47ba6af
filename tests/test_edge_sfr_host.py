"""srx_edge_sfr_* without a GPU.

1. The plain arithmetic of csrc/srx_sfr.hpp (the filters, the radix selection, the line fits from exact sums, the bins, ESF / LSF / DFT /
   crossings) compiled for the host: tests/edge_sfr_host_model.cpp runs it in the kernels' order, built with g++ -fsanitize=address,undefined
   and run as its own process.  Against sr_mi355x.metrics (slanted_edge_esf -> esf_to_mtf -> mtf_at_fraction) on the two golden 200 x 200
   ROIs and eight seeded noisy synthetic edges, both sides, at the tolerances tests/test_gpu_metrics.py holds the device composition to; the
   threshold and the pixel counts must be equal.  No sanitizer report may appear.
2. The selection alone against np.percentile(a, 85), bit for bit: random arrays, heavy ties, all-equal arrays, n = 1, 2, 7, more than 85 %
   zeros.
3. The refusals of the three entry points (decided on the host before any HIP call, in the header's order: the pointers are never
   dereferenced), the scratch query, and the ctypes table."""
import ctypes

import numpy as np
import pytest

import edge_sfr_cases as C
from sr_mi355x import _lib

ROIS = C.rois()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if C.GXX is None:
        pytest.skip("no g++")
    return C.build_model(str(tmp_path_factory.mktemp("sfr_model") / "edge_sfr_host_model"))


def test_wide_integer_helpers(model):
    assert C._run([model, "selftest"]).strip() == "ok"


@pytest.mark.parametrize("side", list(C.SIDES))
@pytest.mark.parametrize("name", list(ROIS))
def test_model_against_metrics(model, tmp_path, name, side):
    ref = C.reference(ROIS[name], side, key=name)
    got = C.run_model(model, tmp_path, ROIS[name], side)
    C.close_to_reference(got, ref)
    assert got["nbin"] == 72 and np.isfinite(got["mtf50"]) and np.isfinite(got["mtf10"])
    # the closed form on exact sums against np.polyfit
    for k in ("m", "b", "m_c", "b_c"):
        assert abs(got[k] - ref[k]) <= 9e-14 * max(1.0, abs(ref[k])), (k, got[k], ref[k])


def test_model_takes_both_orientations(model, tmp_path):
    """the model's own rows_are_x over the inputs: both branches of the fits and of the projection run, and agree with metrics.py"""
    got = {n: C.run_model(model, tmp_path, ROIS[n], "left")["rows_are_x"] for n in ROIS}
    assert set(got.values()) == {0.0, 1.0}
    assert all(bool(v) == C.reference(ROIS[n], "left", key=n)["rows_are_x"] for n, v in got.items())


STATUS_CASES = C.status_cases()


@pytest.mark.parametrize("name", list(STATUS_CASES))
def test_model_statuses_on_thin_and_small_rois(model, tmp_path, name):
    a, want = STATUS_CASES[name]
    for side in C.SIDES:
        got = C.run_model(model, tmp_path, a, side)
        assert got["status"] == want and got["n_edge"] >= 20 and got["zero"] == 0.0
        if want == 0:
            ref = C.reference(a, side)
            assert got["threshold"] == ref["threshold"] and got["n_side"] == ref["n_side"] and 4 <= got["nbin"] == ref["nbin"] < 72
            np.testing.assert_allclose(got["esf_x"], ref["esf_x"], rtol=0, atol=1e-9)
            np.testing.assert_allclose(got["esf_y"], ref["esf_y"], rtol=0, atol=1e-8)
            np.testing.assert_allclose(got["mtf"], ref["mtf"], rtol=0, atol=1e-8)
            for k in ("mtf50", "mtf10"):  # (a short curve may never fall through: nan on both sides)
                v, w = got[k] / C.HR_PITCH, ref[k + "_mm"]
                assert (np.isnan(v) and np.isnan(w)) or abs(v - w) <= 1e-6, (k, v, w)
            nbin = int(got["nbin"])
            assert (got["esf"][:, nbin:] == 0).all() and (got["mtf_raw"][:, nbin // 2:] == 0).all()
        else:
            assert np.isnan(got["esf"]).all() and np.isnan(got["mtf_raw"]).all() and np.isnan(got["mtf50"]) and np.isnan(got["flipped"])
        if want == 2:
            assert got["n_side"] == 0 and np.isnan(got["m"]) and np.isfinite(got["m_c"])
        if want == 4:  # the line is known, its angle too; four bins, of which one is filled
            assert got["nbin"] == 4 and got["hi"] - got["lo"] == 1.0 and got["angle_deg"] in (0.0, 90.0) and got["m"] == 0.0


def test_model_on_non_integer_samples(model, tmp_path):
    roi = C.edge(37, 53, 0.35, seed=5) * 0.75 + 0.3
    for side in C.SIDES:
        C.close_to_reference(C.run_model(model, tmp_path, roi, side), C.reference(roi, side))


def test_model_on_the_zero_plane(model, tmp_path):
    z = C.zero_plane()
    mag = C.magnitude(z)
    assert (mag == 0).mean() > 0.85 and np.percentile(mag, 85) == 0.0
    for side in C.SIDES:
        ref = C.reference(z, side, key="zero_plane")
        got = C.run_model(model, tmp_path, z, side)
        C.close_to_reference(got, ref)
        assert got["threshold"] == 0.0 and got["n_edge"] == (mag > 0).sum()


def test_model_statuses(model, tmp_path):
    const = C.run_model(model, tmp_path, np.full((37, 53), 9.0), "left")
    assert const["status"] == 1 and const["threshold"] == 0.0 and const["n_edge"] == 0 and np.isnan(const["mtf50"]) and np.isnan(const["m"])
    assert np.isnan(const["esf"]).all() and np.isnan(const["mtf_raw"]).all() and const["zero"] == 0.0
    # an 8 x 8 ROI has 9 or 10 pixels above its 85th percentile; a 12 x 12 one 21 or 22, but its distances span fewer than 18 px
    tiny = C.run_model(model, tmp_path, C.edge(8, 8, 0.3, seed=1), "left")
    assert tiny["status"] == 1 and 0 < tiny["n_edge"] < 20 and tiny["threshold"] > 0
    small = C.run_model(model, tmp_path, C.edge(12, 12, 0.3, seed=1), "left")
    assert small["status"] in (0, 2) and small["n_edge"] >= 20
    if small["status"] == 0:
        assert small["nbin"] < 72 and (small["esf"][:, int(small["nbin"]):] == 0).all()


PERCENTILE_CASES = {
    "random_1000": lambda r: r.uniform(0, 300, 1000),
    "random_40000": lambda r: r.uniform(0, 1e-3, 40000),
    "wide_exponents": lambda r: np.exp(r.uniform(-300, 300, 5001)),
    "ties_heavy": lambda r: r.integers(0, 4, 2001).astype(np.float64),
    "ties_at_the_index": lambda r: np.concatenate([r.uniform(0, 1, 84), np.full(10, 1.5), r.uniform(2, 3, 7)]),
    "all_equal": lambda r: np.full(333, 2.75),
    "all_zero": lambda r: np.zeros(100),
    "n1": lambda r: np.array([3.5]),
    "n2": lambda r: np.array([4.0, 1.0]),
    "n7": lambda r: r.uniform(0, 9, 7),
    "zeros_86_percent": lambda r: np.concatenate([np.zeros(860), r.uniform(0.1, 5, 140)]),
    "zeros_up_to_the_index": lambda r: np.concatenate([np.zeros(850), r.uniform(0.1, 5, 151)]),
    "subnormals_and_inf": lambda r: np.concatenate([r.uniform(0, 1, 50) * 5e-324 * 1000, [np.inf] * 8, r.uniform(0, 1, 30)]),
}


@pytest.mark.parametrize("name", list(PERCENTILE_CASES))
def test_selection_equals_np_percentile(model, tmp_path, name):
    rng = np.random.default_rng(sorted(PERCENTILE_CASES).index(name))
    a = PERCENTILE_CASES[name](rng)
    rng.shuffle(a)
    want = np.percentile(a, 85)
    got = C.model_percentile(model, tmp_path, a)
    assert C.bits(got) == C.bits(want), (got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# entry points: refusals and queries
# ---------------------------------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)
ENTRIES = ("srx_edge_sfr_u8", "srx_edge_sfr_f32", "srx_edge_sfr_f64")
OK_ARGS = dict(img=FAKE, B=2, H=37, W=53, row_pitch=53, item_pitch=37 * 53, side=0, sigma=1.5, summary=FAKE, esf=FAKE, mtf=FAKE, status=FAKE, ws=FAKE,
               wsb=1 << 30)


def call(entry, **kw):
    a = dict(OK_ARGS, **kw)
    return getattr(_lib.load(), entry)(a["img"], a["B"], a["H"], a["W"], a["row_pitch"], a["item_pitch"], a["side"], a["sigma"], a["summary"], a["esf"],
                                       a["mtf"], a["status"], a["ws"], a["wsb"], None)


INVALID = {"null_img": dict(img=None), "null_summary": dict(summary=None), "null_status": dict(status=None), "B0": dict(B=0), "B_neg": dict(B=-1),
           "H0": dict(H=0), "W0": dict(W=0), "W_neg": dict(W=-5), "row_pitch_short": dict(row_pitch=52), "item_pitch_short": dict(item_pitch=36 * 53 + 52),
           "side2": dict(side=2), "side_neg": dict(side=-1), "sigma0": dict(sigma=0.0), "sigma_neg": dict(sigma=-1.5), "sigma_nan": dict(sigma=float("nan"))}
UNSUPPORTED = {"pixels": dict(B=1, H=1025, W=1024, row_pitch=1024), "pixels_over_int": dict(B=1, H=1 << 16, W=1 << 16, row_pitch=1 << 16),
               "B65536": dict(B=65536), "radius9": dict(sigma=2.2), "sigma_inf": dict(sigma=float("inf"))}
WORKSPACE = {"null_ws": dict(ws=None), "short_ws": dict(wsb=255), "misaligned_ws": dict(ws=ctypes.c_void_p(4096 + 128)), "zero_ws": dict(wsb=0)}


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals(entry):
    for name, kw in INVALID.items():
        assert call(entry, **kw) == _lib.E_INVALID, name
    for name, kw in UNSUPPORTED.items():
        assert call(entry, **kw) == _lib.E_UNSUPPORTED, name
    for name, kw in WORKSPACE.items():
        assert call(entry, **kw) == _lib.E_WORKSPACE, name
    assert call(entry, B=65536, side=3) == _lib.E_INVALID       # invalid wins over unsupported
    assert call(entry, B=65536, ws=None) == _lib.E_UNSUPPORTED  # and unsupported over the workspace
    need = _lib.load().srx_edge_sfr_scratch_bytes(2, 37, 53)
    assert call(entry, wsb=need - 1) == _lib.E_WORKSPACE
    # the limits themselves are no refusal: with a short workspace these get as far as SRX_E_WORKSPACE
    assert call(entry, B=1, H=1024, W=1024, row_pitch=1024, item_pitch=0, wsb=256) == _lib.E_WORKSPACE
    assert call(entry, B=1, item_pitch=0, sigma=2.1, esf=None, mtf=None, wsb=256) == _lib.E_WORKSPACE  # B = 1: no item pitch; radius 8; esf / mtf optional


def test_scratch_query():
    lib = _lib.load()
    for b, h, w in ((1, 1, 1), (1, 37, 53), (3, 200, 200), (24, 200, 200), (1, 1024, 1024), (1, 1 << 20, 1), (65535, 4, 4)):
        s = lib.srx_edge_sfr_scratch_bytes(b, h, w)
        assert s > 0 and s % 256 == 0 and s >= b * (2 * h * w + C.SUMMARY) * 8, (b, h, w)
    assert lib.srx_edge_sfr_scratch_bytes(3, 200, 200) >= lib.srx_edge_sfr_scratch_bytes(1, 200, 200)
    for b, h, w in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (65536, 4, 4), (1, 1025, 1024), (1, 1 << 16, 1 << 16)):
        assert lib.srx_edge_sfr_scratch_bytes(b, h, w) == 0, (b, h, w)


def test_symbols_are_in_the_ctypes_table():
    import test_abi
    assert set(ENTRIES) | {"srx_edge_sfr_scratch_bytes"} <= set(_lib.symbols())
    assert sorted(_lib.symbols()) == test_abi.header_symbols()
