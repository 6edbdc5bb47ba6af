"""The patch kernel's neighbour-exchange stores (srx_block.hpp's xstore: ds_write_addtid_b32 behind an M0 set-up) and the two forms of its
byte-mosaic G step (the 0/1 count masks tested, or known to be all ones: srx_patch.hpp's gstep_form), on the smallest shape the patch
path takes: 256 x 256 HR from 64 x 64 LR frames at f = 4, two items, five iterations.

Every case is compared with the oracle at the tolerances of tests/test_gpu_parity.py::test_patch_kernel_vs_oracle (HR state 1e-3 DN, MSE
trace rtol 2e-5) and with the tile kernels (HR state 5e-4 DN, trace rtol 2e-6).  Which form of the G step a table of shifts takes is
asked of the library itself (srx_ibp_patch_gstep_for: the function the call reads), so a case that was meant for one form and reaches
the other fails here, not silently.

    case            frames                         G step                   row above the grid (exy: the rowbuf store)
    grid            4 x 4 phases                   masks all ones (2)       yes
    grid_exy0       4 x 4 phases, rows -1/4 px     masks all ones (2)       no
    rows2           2 x 4 phase classes            masks tested (1)         no
    rows2_exy1      2 x 4, the two lower classes   masks tested (1)         yes
    rows3_exy0      3 x 4 phase classes            masks tested (1)         no
    dup             4 x 4 + one phase twice        count plane (0)          yes
    grid_asym       4 x 4, 5 x 5-core PSF          masks all ones (2), tested all the same: the form without the test is the rank-1 kernel's
    grid_full7      4 x 4, full 7 x 7 PSF          as grid_asym
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import sr_mi355x as S  # noqa: E402
from sr_mi355x import _lib, synth  # noqa: E402

F, B, N_ITER = 4, 2, 5
P4 = synth.phase_shifts(4)
ROW = sorted({s[0] for s in P4})  # the four row phases, ascending: integer parts -2, -1, 0, 1 of f s

CASES = {
    # name: (shifts, psf, G-step form, exy)
    "grid": (P4, "gauss", 2, 1),
    "grid_exy0": ([(sy - 0.25, sx) for sy, sx in P4], "gauss", 2, 0),
    "rows2": ([s for s in P4 if s[0] in ROW[1:3]], "gauss", 1, 0),
    "rows2_exy1": ([s for s in P4 if s[0] in ROW[2:4]], "gauss", 1, 1),
    "rows3_exy0": ([s for s in P4 if s[0] in ROW[0:3]], "gauss", 1, 0),
    "dup": (P4 + [P4[5]], "gauss", 0, 1),
    "grid_asym": (P4, "asym", 2, 1),
    "grid_full7": (P4, "full7", 2, 1),
}


def gstep_form(shifts):
    a = np.ascontiguousarray(np.asarray(shifts, dtype=np.float64))
    return _lib.load().srx_ibp_patch_gstep_for(len(a), F, a.ctypes.data_as(_lib._HD))


def test_the_cases_reach_the_forms_they_are_meant_for():
    """Host only: the G-step form and the row above the grid of every case's table (the rank-1 kernel's form: a 7 x 7 PSF keeps the mask test)."""
    for name, (shifts, _, form, exy) in CASES.items():
        assert gstep_form(shifts) == form, name
        assert int(max(np.floor(4 * s[0] + 1e-12) for s in shifts) > 0) == exy, name


def test_gstep_form_of_the_host():
    """The predicate that selects the all-ones form: the flagship's 16 phases take it; a grid with a missing row class has zero rows in its mask;
    15 of the 16 phases are no product grid at all (count plane); an all-ones grid whose shifts are moved by a whole LR pixel stays one."""
    assert gstep_form(P4) == 2
    assert gstep_form([s for s in P4 if s[0] != ROW[0]]) == 1
    assert gstep_form([s for s in P4 if s[1] != ROW[3]]) == 1
    assert gstep_form(P4[:15]) == 0
    assert gstep_form(P4[1:]) == 0
    assert gstep_form([(sy - 0.25, sx - 0.25) for sy, sx in P4]) == 2
    assert gstep_form([(0.1, 0.1), (0.3, 0.1)]) == -1  # no common fraction: no mosaic


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_patch_kernel_exchange_and_gstep(case):
    from oracle import sr_oracle as O
    from test_gpu_parity import ERR_RTOL, IBP_TOL, _patch_case, close
    S.set_precision("f32")
    shifts, psf_name, _, _ = CASES[case]
    psf, lr, saa = _patch_case(F, shifts, B, True, seed=410, psf_name=psf_name)
    hr, errs = S.ibp_batched(lr, shifts, psf, saa, F, N_ITER, 0.5)
    assert S.last_path() == "patch"
    O.set_threads(8)
    try:
        for i in range(B):
            hr_o, err_o = O.ibp(list(lr[i]), shifts, psf, saa[i], F, N_ITER, 0.5)
            close(hr[i].cpu().numpy(), hr_o, IBP_TOL["f32"])
            np.testing.assert_allclose(errs[i].cpu().numpy(), err_o, rtol=ERR_RTOL["f32"])
    finally:
        O.set_threads(1)
    hr_t, e_t = S.ibp_batched(lr, shifts, psf, saa, F, N_ITER, 0.5, flags=S.FLAG_TILES)
    assert S.last_path() == "mosaic"
    assert float((hr - hr_t).abs().max()) < 5e-4
    np.testing.assert_allclose(errs.cpu().numpy(), e_t.cpu().numpy(), rtol=2e-6)
    hr_r, errs_r = S.ibp_batched(lr, shifts, psf, saa, F, N_ITER, 0.5)  # the same bits from call to call
    assert torch.equal(hr_r, hr) and torch.equal(errs_r, errs)
