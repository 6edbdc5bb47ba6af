"""The preconditions of tests/test_gpu_register_edges.py, asserted on the oracle of tests/register_oracle.py alone, and the oracle's own
decision rules against brute force: its tie order against sorted() over every offset, its edge clamping against np.pad(mode='edge'), its
status priority.  The cases are tests/register_edge_cases.py's.  No GPU."""
import itertools

import numpy as np
import pytest

pytest.importorskip("scipy")

import register_edge_cases as C  # noqa: E402
import register_oracle as R  # noqa: E402


def f64(name):
    fr, kw = C.case(name)
    return fr.astype(np.float64), kw


def maps_of(name):
    """per moving frame k: (k, c0, the oracle's score over the search window)"""
    fr, kw = f64(name)
    N, H, W = fr.shape
    ref, search = kw.get("ref", 0), kw.get("search", 2)
    m = R.margin(kw.get("border", 8), search)
    init = np.zeros((N, 2)) if kw.get("init") is None else np.asarray(kw["init"], np.float64)
    for k in range(N):
        if k != ref:
            c0 = tuple(int(v) for v in np.rint(init[k] - init[ref]))
            yield k, c0, C.score_map(fr[k], fr[ref][m:H - m, m:W - m], m, c0, search)


# ---- 1a. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rolls,expect", [("ties", C.TIE_ROLLS, C.TIE_EXPECT), ("ties_total_shift", C.TIE2_ROLLS, C.TIE2_EXPECT)])
def test_tied_maxima_are_the_expected_set_and_clear_of_the_rest(name, rolls, expect):
    fr, kw = C.case(name)
    assert np.array_equal(fr, np.clip(fr, 0, 255)) and fr.shape[1:] == (64, 64)
    m = R.margin(kw["border"], kw["search"])
    assert (m, fr.shape[1] - 2 * m) == ((14, 36) if name == "ties" else (12, 40))
    for (k, c0, smap), roll, want in zip(maps_of(name), rolls, expect):
        top = max(smap.values())
        tied = {d for d, s in smap.items() if s == top}
        assert top == 1.0 and tied == C.tied_offsets(want, c0, kw["search"]), (roll, top, tied)
        assert max(s for d, s in smap.items() if d not in tied) <= top - C.TIE_GAP, roll
        assert C.brute_argmax(smap) == want, roll
        if roll in C.TIE_MAXIMA:
            assert len(tied) == C.TIE_MAXIMA[roll]
    d, score, status, dc = C.oracle(name)
    assert np.array_equal(dc[1:], expect) and np.array_equal(d, dc)
    assert list(status[1:]) == ([0] * 7 if name == "ties" else [2, 2])
    if name == "ties":  # all but one of the nine maxima of the unrolled frame lie on the search boundary; the one inside is kept
        assert sum(1 for (dy, dx) in C.tied_offsets((0, 0), (0, 0), 4) if max(abs(dy), abs(dx)) == 4) == 8
    else:  # ranking the offset instead of the total shift would give (-5, 0) for frame 1 (frame 2's two maxima rank alike either way)
        got = []
        for (k, c0, smap), want in zip(maps_of(name), expect):
            got.append(sorted((-s, abs(dy - c0[0]) + abs(dx - c0[1]), dy - c0[0], dx - c0[1], dy, dx) for (dy, dx), s in smap.items())[0][4:])
        assert got == [(-5, 0), (0, 1)], got


def test_ties_refined_keep_the_integer_and_converge():
    d, score, status, dc = C.oracle("ties_refined")
    assert np.array_equal(dc[1:], C.TIE_EXPECT) and list(status) == [0] * 8
    assert np.abs(d - dc).max() < 1e-9 and np.abs(score - 1.0).max() < 1e-9


def test_oracle_tie_order_against_sorted():
    """R.coarse keeps the first maximum in (|dy| + |dx|, dy, dx): the same as sorted() over every offset, ties and clamped windows included"""
    for name in ("ties", "ties_total_shift", "outside_n0", "huge_init_n0", "flat_reference", "crop16_s4", "singular_on_boundary"):
        fr, kw = f64(name)
        H, W = fr.shape[1:]
        ref, search = kw.get("ref", 0), kw.get("search", 2)
        m = R.margin(kw.get("border", 8), search)
        for k, c0, smap in maps_of(name):
            want = C.brute_argmax(smap)
            got, edge = R.coarse(fr[k], fr[ref][m:H - m, m:W - m], m, c0, search)
            assert got == want, (name, k, got, want)
            assert edge == (search > 0 and max(abs(want[0] - c0[0]), abs(want[1] - c0[1])) == search)


def test_oracle_edge_clamping_against_np_pad():
    for name in ("outside_n0", "halves", "huge_init_n0"):
        fr, kw = f64(name)
        H, W = fr.shape[1:]
        ref, search = kw.get("ref", 0), kw["search"]
        m = R.margin(kw["border"], search)
        left = False
        for k, c0, smap in maps_of(name):
            if max(abs(c0[0]), abs(c0[1])) > 100:  # np.pad by 10^6 samples: the window is one corner sample, the score 0
                assert set(smap.values()) == {0.0}
                left = True
                continue
            assert smap == C.score_map_padded(fr[k], fr[ref][m:H - m, m:W - m], m, c0, search), (name, k)
            left |= max(abs(c0[0]), abs(c0[1])) + search > m
        assert left, name  # a window of the case does leave the frame


def test_oracle_status_priority():
    """1 over 2 over 3: each pair decided on frames that meet both conditions"""
    for name, want in (("singular_on_boundary", 1), ("huge_init", 1), ("boundary_not_converged", 2), ("huge_init_n0", 2)):
        fr, kw = f64(name)
        d, score, status, dc = C.oracle(name)
        assert list(status[1:]) == [want] * (len(status) - 1), (name, status)
    # singular and on the boundary: the same frames at n_iter = 0 are on the boundary only
    fr, kw = f64("singular_on_boundary")
    d0 = R.register_item(fr, **dict(kw, n_iter=0))
    assert d0[2][1] == 2 and np.array_equal(d0[3][1], [2.0, 0.0])
    assert np.array_equal(C.oracle("singular_on_boundary")[0][1], [2.0, 0.0])
    # on the boundary and not converged: inside a wider search the same call is not converged only
    fr, kw = f64("boundary_not_converged")
    assert R.register_item(fr, **dict(kw, search=3))[2][1] == 3
    steps = C.clamped_steps("boundary_not_converged", 1)
    assert np.abs(steps[0, 1]).max() >= 10 * 1e-4
    # singular and not converged: a singular frame never takes a step, so 3 cannot apply to it; n_iter = 0 is never 3
    assert 3 not in C.oracle("flat_moving")[2] and C.oracle("flat_moving")[2][1] == 1


# ---- 1b. the block regimes of the coarse kernel -----------------------------------------------------------------------------------------
def test_coarse_cases_reach_their_regimes():
    for name in C.COARSE_REGIME_CASES:
        fr, kw = C.case(name)
        assert kw["border"] == 0 and kw["n_iter"] == 0
        h, w = C.crop_of(fr.shape, kw["search"], 0)
        p = C.make_plan(h, w, kw["search"])
        if name.startswith("chunk_"):
            want_w = int(name.split("_")[1])
            assert (h, w) == (33, want_w) and fr.shape[0] == 3
            assert (p["cgx"], w % C.CW) == {63: (1, 63), 64: (1, 0), 65: (2, 1)}[want_w]  # a partial chunk, a full one, one column over
            assert (p["noff"], p["groups"], 256 - p["noff"] * p["groups"]) == ((1, 256, 0) if kw["search"] == 0 else (81, 3, 13))
            assert (p["cgy"], p["crow"]) == (3, 16)  # the last block row is one row high
        elif name == "crop16_s4":
            assert fr.shape == (3, 28, 28) and (h, w) == (16, 16) and (p["noff"], p["cgx"], p["cgy"]) == (81, 1, 1)
        elif name == "crop17x16_s2":
            assert (h, w) == (17, 16) and (p["cgx"], p["cgy"], p["crow"]) == (1, 2, 16) and h - p["crow"] == 1
            assert (p["noff"], p["groups"], 256 - p["noff"] * p["groups"]) == (25, 10, 6)
        else:
            assert fr.shape == (2, 160, 2200) and (h, w) == (152, 2192)
            assert (p["cgx"], p["crow"], p["cgy"]) == (35, 32, 5)  # two 16-row chunks per coarse block
        d, score, status, dc = C.oracle(name)
        assert np.array_equal(d, dc) and 3 not in status


def test_refinement_strip_cases():
    for name, (ggx, last) in zip(C.STRIP_CASES, ((1, 255), (1, 256), (2, 1))):
        fr, kw = C.case(name)
        h, w = C.crop_of(fr.shape, kw["search"], kw["border"])
        p = C.make_plan(h, w, kw["search"])
        assert h == 41 and w == int(name[6:]) and (p["ggx"], w - (p["ggx"] - 1) * C.GW) == (ggx, last)
        assert (p["ggy"], p["grow"]) == (3, 14)  # 14 + 14 + 13 rows
        assert list(C.oracle(name)[2]) == [0, 0, 0]


# ---- 1c. init ---------------------------------------------------------------------------------------------------------------------------
def test_init_rounds_half_to_even():
    assert np.array_equal(np.rint(np.asarray(C.HALVES)), C.HALVES_EXPECT)
    t = np.asarray(C.HALVES) + 1.0
    assert np.array_equal(np.rint(t - t[3]), C.HALVES_REF3_EXPECT)
    for name, want, ref in (("halves", C.HALVES_EXPECT, 0), ("halves_ref3", C.HALVES_REF3_EXPECT, 3)):
        fr, kw = C.case(name)
        assert all(np.array_equal(fr[0], f) for f in fr) and kw["search"] == 0 and kw["n_iter"] == 0 and kw.get("ref", 0) == ref
        d, score, status, dc = C.oracle(name)
        assert np.array_equal(d, want) and list(status) == [0] * 6 and score[ref] == 1.0
    # the two neighbours of one half differ by one ulp from it and round apart
    assert C.HALVES[5][0] == np.nextafter(0.5, 0.0) and C.HALVES[5][1] == np.nextafter(0.5, 1.0)


def test_outside_windows_leave_the_frame_and_find_the_shift():
    for name in ("outside_n0", "outside_n10"):
        fr, kw = C.case(name)
        assert fr.shape == (3, 96, 120) and R.margin(kw["border"], kw["search"]) == 4
        d, score, status, dc = C.oracle(name)
        assert np.array_equal(dc[1:], [[7, -6], [-7, 5]]) and list(status) == [0, 0, 0]
        if name == "outside_n10":
            assert np.abs(d - np.asarray(C.OUTSIDE_SHIFTS)).max() < 0.05
    # the coarse window reaches 7 + 2 - 4 = 5 samples past the frame; the refined taps pass it as well
    assert max(abs(v) for s in C.OUTSIDE_SHIFTS for v in s) + 2 > 4 + 2


def test_largest_accepted_init():
    assert np.all(np.abs(np.asarray(C.HUGE_INIT)) <= 1e6)
    for name, st in (("huge_init", 1), ("huge_init_n0", 2)):
        fr, kw = C.case(name)
        assert fr.shape == (3, 48, 56)
        d, score, status, dc = C.oracle(name)
        assert np.array_equal(d, C.HUGE_EXPECT) and np.array_equal(score, [1.0, 0.0, 0.0]) and list(status) == [0, st, st]
    for name, init in C.REFUSED_INITS.items():
        v = np.asarray(init)
        assert not np.all(np.abs(v - v[0]) <= 1e6), name


# ---- 1d. constant content ---------------------------------------------------------------------------------------------------------------
def test_constant_content():
    fr, kw = C.case("flat_reference")
    assert np.all(fr[0] == 77) and kw["n_iter"] == 0
    d, score, status, _ = C.oracle("flat_reference")
    assert np.array_equal(d, np.zeros((3, 2))) and np.array_equal(score, [1.0, 0.0, 0.0]) and list(status) == [0, 0, 0]
    fr, kw = C.case("flat_moving")
    assert np.all(fr[1] == 77) and fr[0].std() > 10
    d, score, status, _ = C.oracle("flat_moving")
    assert np.array_equal(d[1], [0.0, 0.0]) and score[1] == 0.0 and list(status) == [0, 1, 0]


# ---- 2. refinement ----------------------------------------------------------------------------------------------------------------------
def test_refinement_preconditions():
    fr = C.refine_frames().astype(np.float64)
    assert fr.shape == (3, 96, 112)
    # frame 1's first two raw steps exceed 0.6 px on both axes, so both are clamped to 0.5
    r1 = C.raw_step(fr, 1, (0.0, 0.0), **C.REFINE_KW)
    r2 = C.raw_step(fr, 1, (0.5, -0.5), **C.REFINE_KW)
    print("raw steps of frame 1:", r1, r2)
    assert r1[0] > 0.6 and r1[1] < -0.6 and r2[0] > 0.6 and r2[1] < -0.6
    steps = C.clamped_steps("refine_2", 10)  # tol = 0: every step is taken
    assert np.array_equal(steps[0, 1], [0.5, -0.5]) and np.array_equal(steps[1, 1], [0.5, -0.5])
    assert np.array_equal(steps[0, 1], np.clip(r1, -0.5, 0.5)) and np.array_equal(steps[1, 1], np.clip(r2, -0.5, 0.5))
    # the third is not clamped and is the raw step at (1, -1)
    assert np.abs(steps[2, 1] - C.raw_step(fr, 1, (1.0, -1.0), **C.REFINE_KW)).max() < 1e-12 and np.abs(steps[2, 1]).max() < 0.5
    big = np.abs(steps).max(axis=2)  # [step, frame]
    print("max |step| per iteration, frames 1 and 2:", big[:, 1], big[:, 2])
    for k in (1, 2):
        # status 3 at n_iter = 1, 2: the last step is at least 10 tol; status 0 at n_iter = 10: the first step below tol is below tol / 10
        assert big[0, k] >= 1e-3 and big[1, k] >= 1e-3
        first = int(np.argmax(big[:, k] < 1e-4))
        assert 0 < first < 10 and big[first, k] <= 1e-5 and np.all(big[:first, k] > 1e-4), (k, big[:, k])
        # tol = 1.0 stops after the first step
        assert big[0, k] < 1.0


def test_refinement_table_on_the_oracle():
    for i, (n_iter, tol, exact, st) in enumerate(C.REFINE_ROWS):
        d, score, status, dc = C.oracle(f"refine_{i}")
        assert np.array_equal(dc, np.zeros((3, 2))) and tuple(status[1:]) == st, (i, status)
        if exact is not None:
            assert np.array_equal(d[1], exact), (i, d[1])
    a, b = C.oracle("refine_4"), C.oracle("refine_0")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    d = C.oracle("refine_3")[0]
    assert np.abs(d - np.asarray(C.REFINE_SHIFTS)).max() < 0.01
    assert np.array_equal(C.oracle("refine_5")[0], np.zeros((3, 2)))


def test_frame_count_cases():
    fr, kw = C.case("n2")
    assert fr.shape[0] == 2 and list(C.oracle("n2")[2]) == [0, 0]
    for name, ref in (("n32", 0), ("n32_ref_last", 31)):
        fr, kw = C.case(name)
        init = np.asarray(kw["init"])
        assert fr.shape == (32, 48, 56) and kw["ref"] == ref and np.array_equal(init, np.rint(init))
        d, score, status, dc = C.oracle(name)
        if ref == 0:  # the coarse stage stays at the start it is given
            assert list(status) == [0] * 32 and np.array_equal(dc, init)
        else:  # two roundings apart, a start can be one pixel off: the search (1) finds the shift on its boundary
            assert set(status) == {0, 2} and np.abs(dc - (init - init[ref])).max() == 1
        last = 31 if ref == 0 else 30  # the last entry of the start table that is used
        assert np.all((init - init[ref])[last] != 0)
        assert np.abs(d - (C._n32_shifts() - C._n32_shifts()[ref])).max() < 0.05
    # the starts are distinct enough that a frame started from another frame's entry is found elsewhere (search 1)
    init = np.asarray(C.case("n32")[1]["init"])
    assert len({tuple(v) for v in init}) >= 12
    for i, name in enumerate(C.B3_CASES):
        fr, kw = C.case(name)
        assert fr.shape == (3, 48, 56) and kw["ref"] == 1
        d, score, status, _ = C.oracle(name)
        assert list(status) == [0, 0, 0] and np.array_equal(d[1], [0.0, 0.0])
    for a, b in itertools.combinations(C.B3_CASES, 2):
        assert np.abs(C.oracle(a)[0] - C.oracle(b)[0]).max() > 0.01


# ---- 3. batches -------------------------------------------------------------------------------------------------------------------------
def test_batches_cross_the_prefilter_regimes():
    hp = C.BATCH_HW + 2 * R.NPAD
    assert hp == 88
    for B in C.BATCHES:
        nf = B * (C.BATCH_N - 1)
        assert nf == {255: 1020, 256: 1024, 512: 2048}[B]
        assert C.prefilter_regime(nf, hp, hp) == C.BATCH_REGIME[B]
    # the thresholds themselves: one moving frame fewer changes the regime
    assert C.prefilter_regime(1023, hp, hp) == (32, 1) and C.prefilter_regime(2047, hp, hp) == (64, 1)
    import prims_edge_cases as P
    for nf in (1020, 1023, 1024, 2047, 2048):
        assert C.prefilter_regime(nf, hp, hp) == P.prefilter_regime(nf, hp, hp)
    assert C.LIMIT_B * (2 - 1) == 65535 and C.limit_items().shape == (16, 2, 20, 20)
    assert C.crop_of((20, 20), **C.LIMIT_KW) == (16, 16)
    assert C.prefilter_regime(16, 44, 44) == (32, 1) and C.prefilter_regime(65535, 44, 44) == (256, 8)


def test_batch_items_differ_and_register():
    checked = sorted(set().union(*(C.batch_checked(B) for B in C.BATCHES)) | set().union(*(C.batch_singles(B) for B in C.BATCHES)))
    assert len(checked) < 48
    res = {i: C.batch_oracle(i) for i in checked}
    for i, (d, score, status, dc) in res.items():
        assert list(status) == [0] * C.BATCH_N, (i, status)
        assert np.abs(d - np.asarray(C.NOMINAL_5)).max() < 0.45
    worst = min(np.abs(res[a][0] - res[b][0]).max() for a, b in itertools.combinations(checked, 2))
    print(f"closest pair of compared items: {worst:.4f} px")
    assert worst > 0.01
    lim = [R.register_item(f.astype(np.float64), **C.LIMIT_KW) for f in C.limit_items()]
    assert min(np.abs(a[0] - b[0]).max() for a, b in itertools.combinations(lim, 2)) > 0.01
    assert all(s[2][1] in (0, 3) for s in lim)
