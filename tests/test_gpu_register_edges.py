"""Registration (srx_register_*, srx_register_u8_*: include/srx.h, csrc/srx_register.hpp) at its decision edges and in the batches the
patch-wise path sends it, against the independent oracle of tests/register_oracle.py.  The cases, their expected values and the oracle's
results are tests/register_edge_cases.py's; tests/test_register_edges_host.py asserts their preconditions without a GPU.

Every case runs in four forms at the C ABI -- srx_register_f32 / _f64 on the converted frames, srx_register_u8_f32 / _f64 on the bytes --
with outputs pre-filled with NaN / -1, and the byte form must return the float form's bits.  Tolerances are tests/test_gpu_register.py's:
shifts 1e-8 (f64) / 1e-3 px (f32), score 1e-10 / 1e-4, status equal; what the header states exactly is compared with np.array_equal.
Each comparison prints its deviation (pytest -s), the figures of profiles/README.md."""
import ctypes

import numpy as np
import pytest
import torch

import register_edge_cases as C
import register_oracle as R
from sr_mi355x import _lib, api
from test_gpu_register_u8 import DT, EB, call_abi, on_device, run

pytestmark = pytest.mark.gpu

FORMS = [pytest.param(kind, prec, id=f"{'u8_' if kind == 'u8' else ''}{prec}") for kind, prec in C.FORMS]
WORST = {}  # form -> [largest shift deviation, largest score deviation] against the oracle, over the process


def fn_name(kind):
    return "srx_register_u8" if kind == "u8" else "srx_register"


def both(kind, prec, fr, **kw):
    """the form's (shifts, score, status) [B, N, ..] on the host; a byte form is also held to the bits of its float form"""
    x = on_device(fr if fr.ndim == 4 else fr[None])
    got = run(kind, prec, x, **kw)
    if kind == "u8":
        want = run("float", prec, x, **kw)
        for g, w, what in zip(got, want, ("shifts", "score", "status")):
            assert np.array_equal(g, w), (what, g, w)
    return got


def against(kind, prec, got, want, label):
    """one item (shifts [N, 2], score [N], status [N]) against the oracle's (d, score, status, d_coarse)"""
    d, s, st = got
    assert np.array_equal(st, want[2]), (label, st, want[2])
    dd, ds = float(np.abs(d - want[0]).max()), float(np.abs(s - want[1]).max())
    w = WORST.setdefault(f"{kind}_{prec}", [0.0, 0.0])
    w[0], w[1] = max(w[0], dd), max(w[1], ds)
    print(f"{label} [{kind} {prec}]: max |shift - oracle| = {dd:.3e} px, max |score - oracle| = {ds:.3e}")
    assert dd <= C.TOL_SHIFT[prec], (label, d, want[0])
    assert ds <= C.TOL_SCORE[prec], (label, s, want[1])


def check_case(kind, prec, name):
    fr, kw = C.case(name)
    got = tuple(v[0] for v in both(kind, prec, fr, **kw))
    want = C.oracle(name)
    against(kind, prec, got, want, name)
    ref = kw.get("ref", 0)
    assert np.array_equal(got[0][ref], [0.0, 0.0]) and got[1][ref] == 1.0 and got[2][ref] == 0
    if kw.get("n_iter", 10) == 0:  # the coarse integer, exactly, and never 'not converged'
        assert np.array_equal(got[0], want[3]), (name, got[0], want[3])
        assert 3 not in got[2]
    return got


def teardown_module(module):
    for form, (dd, ds) in sorted(WORST.items()):
        print(f"\nworst against the oracle [{form}]: shift {dd:.3e} px, score {ds:.3e}")


# ---- 1. the coarse stage alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,prec", FORMS)
def test_coarse_ties(kind, prec):
    d, s, st = check_case(kind, prec, "ties")
    assert np.array_equal(d[1:], C.TIE_EXPECT) and list(st) == [0] * 8
    d, s, st = check_case(kind, prec, "ties_total_shift")
    assert np.array_equal(d[1:], C.TIE2_EXPECT) and list(st) == [0, 2, 2]
    d, s, st = check_case(kind, prec, "ties_refined")
    assert list(st) == [0] * 8 and np.abs(d[1:] - np.asarray(C.TIE_EXPECT)).max() <= C.TOL_SHIFT[prec]


@pytest.mark.parametrize("kind,prec", FORMS)
@pytest.mark.parametrize("name", C.COARSE_REGIME_CASES)
def test_coarse_block_regimes(name, kind, prec):
    check_case(kind, prec, name)


@pytest.mark.parametrize("kind,prec", FORMS)
def test_init_rounds_half_to_even(kind, prec):
    d, _, st = check_case(kind, prec, "halves")
    assert np.array_equal(d, C.HALVES_EXPECT) and list(st) == [0] * 6
    d, _, st = check_case(kind, prec, "halves_ref3")
    assert np.array_equal(d, C.HALVES_REF3_EXPECT) and list(st) == [0] * 6


@pytest.mark.parametrize("kind,prec", FORMS)
@pytest.mark.parametrize("name", ["outside_n0", "outside_n10"])
def test_windows_that_leave_the_frame(name, kind, prec):
    check_case(kind, prec, name)


@pytest.mark.parametrize("kind,prec", FORMS)
def test_largest_accepted_init(kind, prec):
    d, s, st = check_case(kind, prec, "huge_init")
    assert np.array_equal(d, C.HUGE_EXPECT) and np.array_equal(s, [1.0, 0.0, 0.0]) and list(st) == [0, 1, 1]
    d, s, st = check_case(kind, prec, "huge_init_n0")
    assert np.array_equal(d, C.HUGE_EXPECT) and np.array_equal(s, [1.0, 0.0, 0.0]) and list(st) == [0, 2, 2]


def raw_call(kind, prec, x, ws, ws_bytes, **kw):
    """-> (return code, shifts, score, status) with the outputs pre-filled as run() fills them; x: the form's own frames"""
    B, N = x.shape[:2]
    shifts = torch.full((B, N, 2), float("nan"), dtype=torch.float64, device="cuda")
    score = torch.full((B, N), float("nan"), dtype=torch.float64, device="cuda")
    status = torch.full((B, N), -1, dtype=torch.int32, device="cuda")
    rc = call_abi(fn_name(kind), prec, x, shifts, score, status, ws, ws_bytes, **kw)
    torch.cuda.synchronize()
    return rc, shifts.cpu().numpy(), score.cpu().numpy(), status.cpu().numpy()


def untouched(shifts, score, status):
    return bool(np.all(np.isnan(shifts)) and np.all(np.isnan(score)) and np.all(status == -1))


@pytest.mark.parametrize("kind,prec", FORMS)
def test_refused_init_leaves_the_outputs_untouched(kind, prec):
    fr, kw = C.case("huge_init")
    x = on_device(fr[None])
    if kind == "float":
        x = x.to(DT[prec])
    need = _lib.load().srx_register_workspace_bytes(EB[prec], 1, 3, fr.shape[1], fr.shape[2], kw["search"])
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for name, init in C.REFUSED_INITS.items():
        rc, *out = raw_call(kind, prec, x, api._p(ws), need, **dict(kw, init=init))
        assert rc == _lib.E_INVALID and untouched(*out), (name, rc)
    rc, *out = raw_call(kind, prec, x, api._p(ws), need, **kw)  # the accepted side of the bound, through the same path
    assert rc == _lib.OK and np.array_equal(out[0][0], C.HUGE_EXPECT)


@pytest.mark.parametrize("kind,prec", FORMS)
def test_constant_content(kind, prec):
    d, s, st = check_case(kind, prec, "flat_reference")
    assert np.array_equal(d, np.zeros((3, 2))) and np.array_equal(s, [1.0, 0.0, 0.0]) and list(st) == [0, 0, 0]
    d, s, st = check_case(kind, prec, "flat_moving")
    assert s[1] == 0.0 and st[1] == 1 and np.array_equal(d[1], [0.0, 0.0])


# ---- 2. refinement: steps, clamp, status ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,prec", FORMS)
def test_refinement_steps_clamp_and_status(kind, prec):
    res = []
    for i, (n_iter, tol, exact, status) in enumerate(C.REFINE_ROWS):
        d, s, st = check_case(kind, prec, f"refine_{i}")
        assert tuple(st[1:]) == status, (n_iter, tol, st)
        if exact is not None:
            assert np.array_equal(d[1], exact), (n_iter, tol, d[1])
        res.append((d, s, st))
    assert np.array_equal(res[5][0], np.zeros((3, 2)))
    # tol = 1.0 stops every frame after its first step: the shifts and scores of n_iter = 1, with status 0
    assert np.array_equal(res[4][0], res[0][0]) and np.array_equal(res[4][1], res[0][1])


@pytest.mark.parametrize("kind,prec", FORMS)
def test_status_priority(kind, prec):
    d, s, st = check_case(kind, prec, "singular_on_boundary")
    assert st[1] == 1 and np.array_equal(d[1], [2.0, 0.0])  # singular over boundary; the coarse shift kept exactly
    d, s, st = check_case(kind, prec, "boundary_not_converged")
    assert st[1] == 2  # boundary over not converged


@pytest.mark.parametrize("kind,prec", FORMS)
@pytest.mark.parametrize("name", C.STRIP_CASES)
def test_refinement_strips(name, kind, prec):
    check_case(kind, prec, name)


@pytest.mark.parametrize("kind,prec", FORMS)
@pytest.mark.parametrize("name", ["n2", "n32", "n32_ref_last"])
def test_frame_counts(name, kind, prec):
    check_case(kind, prec, name)


@pytest.mark.parametrize("kind,prec", FORMS)
def test_three_items_with_ref_1(kind, prec):
    frs = [C.case(n)[0] for n in C.B3_CASES]
    kw = C.case(C.B3_CASES[0])[1]
    got = both(kind, prec, np.stack(frs), **kw)
    for i, name in enumerate(C.B3_CASES):
        against(kind, prec, tuple(v[i] for v in got), C.oracle(name), name)
        assert np.array_equal(got[0][i, 1], [0.0, 0.0]) and got[1][i, 1] == 1.0 and got[2][i, 1] == 0


# ---- 3. batches across the prefilter regimes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,prec", FORMS)
@pytest.mark.parametrize("B", C.BATCHES)
def test_batches_across_the_prefilter_regimes(B, kind, prec):
    fr = C.batch_frames(B)
    x = on_device(fr)
    a = run(kind, prec, x, **C.BATCH_KW)
    b = run(kind, prec, x, **C.BATCH_KW)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)  # two runs, identical bits
    if kind == "u8":
        for u, v in zip(a, run("float", prec, x, **C.BATCH_KW)):
            assert np.array_equal(u, v)
    worst = [0.0, 0.0]
    for i in C.batch_checked(B):
        d_o, s_o, st_o, _ = C.batch_oracle(i)
        assert np.array_equal(a[2][i], st_o), (i, a[2][i], st_o)
        dd, ds = float(np.abs(a[0][i] - d_o).max()), float(np.abs(a[1][i] - s_o).max())
        worst = [max(worst[0], dd), max(worst[1], ds)]
        assert dd <= C.TOL_SHIFT[prec] and ds <= C.TOL_SCORE[prec], (i, dd, ds)
    w = WORST.setdefault(f"{kind}_{prec}", [0.0, 0.0])
    w[0], w[1] = max(w[0], worst[0]), max(w[1], worst[1])
    print(f"B = {B} [{kind} {prec}]: max |shift - oracle| = {worst[0]:.3e} px, max |score - oracle| = {worst[1]:.3e}")
    for i in C.batch_singles(B):
        one = run(kind, prec, on_device(fr[i:i + 1]), **C.BATCH_KW)
        for u, v in zip(a, one):
            assert np.array_equal(u[i:i + 1], v), i


def test_the_largest_batch():
    """B (N - 1) = 65535, the largest z extent of a grid: the first and the last sixteen items carry the bits of a sixteen-item call"""
    items = C.limit_items()
    x16 = on_device(items)
    want = run("u8", "f32", x16, **C.LIMIT_KW)
    assert np.all(np.isfinite(want[0])) and np.all(np.isfinite(want[1]))
    x = x16.repeat(4096, 1, 1, 1)[:C.LIMIT_B].contiguous()
    assert x.shape[0] * (x.shape[1] - 1) == 65535
    got = run("u8", "f32", x, **C.LIMIT_KW)  # asserts SRX_OK
    for g, w in zip(got, want):
        assert np.array_equal(g[:16], w)
        assert np.array_equal(g[-16:], np.concatenate([w[15:], w[:15]]))  # item 65519 is item 15 of the sixteen
    for i in range(16):
        against("u8", "f32", tuple(v[i] for v in want), R.register_item(items[i].astype(np.float64), **C.LIMIT_KW), f"limit item {i}")


@pytest.mark.parametrize("kind,prec", FORMS)
def test_one_item_past_the_largest_batch_is_refused(kind, prec):
    B, N, H, W = C.LIMIT_B + 1, 2, 20, 20
    x = torch.zeros((B, N, H, W), dtype=torch.uint8 if kind == "u8" else DT[prec], device="cuda")
    rc, *out = raw_call(kind, prec, x, ctypes.c_void_p(None), 0, **C.LIMIT_KW)
    assert rc == _lib.E_UNSUPPORTED and untouched(*out), rc
