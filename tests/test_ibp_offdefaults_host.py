"""What tests/test_gpu_ibp_offdefaults.py relies on, checked without a GPU (tests/offdefaults_cases.py holds the cases):

  * every case goes to the kernel it is meant for (srx_ibp_path_for is host arithmetic), in both precisions, under every flag the GPU
    module passes and with the 7 x 7 PSF, so a routing change cannot quietly move a case to another kernel;
  * the reference alone makes the clip work: after 4 iterations at least 1 % of the oracle's pixels are exactly 0.0, at least 1 % exactly
    255.0, and at least 0.1 % started strictly inside (0, 255) and ended on a bound (measured over all cases, both PSFs: 2.6 ... 7.2 % per
    bound; 0.32 ... 1.7 % moved at step 0.3 and 1.1 ... 5.2 % at step 1.0);
  * the clip test's allowance is sound for the reference itself: the oracle started from an image perturbed by a tolerance (1e-3, 1e-8)
    leaves the bound only where the unperturbed value before the clip is within that tolerance of it, on at most 0.5 % of the clipped
    pixels (measured: at most 1 pixel of more than 1000);
  * the counts the z_* cases are there for, from numpy alone: C = 15 with M = 3825 (the packed 16-bit operand's limit), C = 16 with
    M < 4096 (the count alone leaves the packed form), C = 17.
"""
import numpy as np
import pytest

import offdefaults_cases as C

CASES = sorted(C.CASES)


@pytest.fixture(scope="module", autouse=True)
def release_references():
    """the cached inputs and oracle runs (some tens of MB) go when the module is done: nothing later in the session runs beside them"""
    yield
    C.reference.cache_clear()
    C.inputs.cache_clear()


@pytest.mark.parametrize("case", CASES)
def test_routes(case):
    c = C.CASES[case]
    for prec in ("f32", "f64"):
        for flags, want in c["routes"][prec]:
            assert C.path_for(prec, case, "gauss", flags) == want, (prec, hex(flags))
        assert C.path_for(prec, case, "asym") == c["asym"][prec], prec
    assert c["routes"]["f32"][0][0] == C.AUTO and len(c["shifts"]) >= 15
    assert len({want for _, want in c["routes"]["f32"]}) == len(c["routes"]["f32"])  # every flagged run is another kernel


def test_every_route_is_met():
    met = {want for c in C.CASES.values() for prec in ("f32", "f64") for _, want in c["routes"][prec]}
    assert met == {"patch", "stile", "ctile", "ztile", "dtile", "atile", "mosaic", "btile", "fused", "composed"}
    assert {"ztile", "patch", "dtile", "btile", "mosaic"} <= {c["asym"]["f32"] for c in C.CASES.values()}  # the 7 x 7 forms


def test_per_item_tables_stay_on_the_case_route():
    for prec, want in (("f32", "btile"), ("f64", "fused")):
        assert [C.path_for(prec, "b_n15", "gauss", shifts=t) for t in C.PER_ITEM_TABLES] == [want, want]
    assert np.array_equal(C.PER_ITEM_TABLES[0], np.asarray(C.CASES["b_n15"]["shifts"]))
    assert not np.array_equal(C.PER_ITEM_TABLES[0], C.PER_ITEM_TABLES[1])


def test_rough_frames_are_8_bit_with_saturated_corners():
    lr, init = C.rough(C.SEED, 5, 12, 14, 2)
    assert lr.shape == (5, 12, 14) and init.shape == (24, 28)
    assert np.array_equal(lr, lr.astype(np.uint8)) and ((lr <= 30) | (lr >= 225)).all()
    assert (lr[:, :4, :4] == 255).all() and (lr[:, -4:, -4:] == 0).all()
    assert init.min() == 0.0 and init.max() == 255.0 and 0.1 < ((init == 0.0) | (init == 255.0)).mean() < 0.35
    lr2, init2 = C.rough(C.SEED + 1, 5, 12, 14, 2)
    assert not np.array_equal(lr, lr2) and not np.array_equal(init, init2)


@pytest.mark.parametrize("psf_name", sorted(C.PSFS))
@pytest.mark.parametrize("case", CASES)
def test_the_reference_clips(case, psf_name):
    c = C.CASES[case]
    lr, init = C.inputs(case)
    for step in C.STEPS:
        ref = C.reference(case, psf_name, step)
        assert np.array_equal(np.clip(ref["v"], 0.0, 255.0), ref["hr"])  # v is the oracle's own value before its last clip
        at0, at255, moved = C.clip_shares(case, ref)
        print(f"{case} {psf_name} step {step}: {at0:.4f} at 0.0, {at255:.4f} at 255.0, {moved:.4f} moved from inside to a bound")
        assert at0 >= 0.01 and at255 >= 0.01 and moved >= 0.001, (psf_name, step, at0, at255, moved)
        rng = np.random.default_rng(5)
        for tol in (1e-3, 1e-8):
            start = np.clip(init + rng.uniform(-tol, tol, init.shape), 0.0, 255.0)
            hr = C.oracle_ibp(lr, c["shifts"], C.PSFS[psf_name](), start, c["f"], C.N_ITER, step)[0]
            clipped, near, far = C.clip_misses(hr, ref, tol)
            assert far == 0 and near <= C.CLIP_EXCEPTIONS * clipped, (psf_name, step, tol, clipped, near, far)


def test_clip_misses_counts_what_it_says():
    ref = {"hr": np.array([0.0, 0.0, 0.0, 255.0, 255.0, 100.0]), "v": np.array([-5.0, -5e-4, -5.0, 255.0004, 300.0, 100.0])}
    assert C.clip_misses(ref["hr"], ref, 1e-3) == (5, 0, 0)
    assert C.clip_misses(np.array([0.0, 1e-4, 1e-4, 254.9999, 256.0, 0.0]), ref, 1e-3) == (5, 2, 2)


@pytest.mark.parametrize("case,count,total,equal", [("z_c15", 15, 3825, 15), ("z_c16", 16, 4080, 16), ("z_c17", 17, 4335, 15)])
def test_counts_at_the_packed_operand_limit(case, count, total, equal):
    """k_ztile_pack / k_ctile_pack take (C << 12 | M) while every C < 16 and every M < 4096"""
    Cp, M = C.far_field_planes(case)
    assert Cp.max() == count and M.max() == total == 255 * count
    assert M[Cp == count].max() == total  # on the saturated corner
    shifts = C.CASES[case]["shifts"]
    assert len(shifts) == 32 and max(shifts.count(s) for s in set(shifts)) == equal  # (equal shifts; the count is per pixel)
