"""k_ibp_patch with resident rows (csrc/srx_patch.hpp, resident_rows()): the instantiations of a full phase grid with a rank-1 PSF keep
rows 0 .. 15 of every wave's 64 x 64 block of the pre-update state in registers from stage A to the update and park rows 16 .. 63 only; the
other instantiations park all 64 rows as before.  Both sides of that boundary, against the CPU oracle:

  n_iter 1, 2, 3   the first park with resident rows, the hand-over of the updated rows 0 .. 15 to the next iteration, the steady state;
                   each out of place and with hr_out aliasing hr_init (the parking layout lives in the output buffer);
  three patches    8-bit frames (the byte mosaic), the same kind with one non-integer sample (the float twin), and 8-bit frames under a
                   start image of 0 / 255 squares, which drives pixels onto both clip bounds in rows 0 .. 15 and in rows 16 .. 63 of the
                   blocks (asserted on the oracle's result);
  five operators   the full 4 x 4 phase grid with the Gaussian PSF (resident rows), the grid with one frame dropped (a count plane) and a
                   3 x 4 product grid (0 / 1 masks that are tested), the 5 x 5-core and the full 7 x 7 PSF (all of them park everything).

Bounds: tests/test_gpu_parity.py's for the patch route, 1e-3 DN on the state and 2e-5 relative on the MSE trace; a pixel the oracle puts
on 0.0 or 255.0 is exactly there; two runs of one call give the same bits; the output sits between guard bands (tests/memguard.py)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import memguard as MG  # noqa: E402
import sr_mi355x as S  # noqa: E402
from sr_mi355x import synth  # noqa: E402

F, PN, B = 4, 256, 3
TOL, ERR_RTOL = 1e-3, 2e-5  # tests/test_gpu_parity.py: IBP_TOL["f32"], ERR_RTOL["f32"]
GRID16 = synth.phase_shifts(4)
CFGS = {
    # name: (shifts, PSF)
    "grid16_gauss": (GRID16, synth.gaussian_psf),
    "grid15_gauss": ([s for i, s in enumerate(GRID16) if i != 6], synth.gaussian_psf),
    "grid12_gauss": ([s for s in GRID16 if s[0] > -0.3], synth.gaussian_psf),
    "grid16_core5": (GRID16, synth.asymmetric_psf),
    "grid16_full7": (GRID16, synth.full_support_psf),
}


@functools.lru_cache(maxsize=None)
def inputs(cfg):
    """(lr [B, N, 64, 64], hr0 [B, 256, 256]) as read-only float64 arrays"""
    from oracle import sr_oracle as O
    shifts, psf = CFGS[cfg][0], CFGS[cfg][1]()
    O.set_threads(8)
    try:
        truths = [synth.truth_image(PN, PN, seed=700 + i) for i in range(B)]
        lr = np.stack([synth.sensor_frames(np.stack([O.forward_model(t, psf, s, F) for s in shifts]), seed=750 + i) for i, t in enumerate(truths)])
        assert np.array_equal(lr, np.rint(lr)) and lr.min() >= 0 and lr.max() <= 255
        lr[1, 3, 20, 41] += 0.5  # one sample that is no integer: the whole patch takes the float mosaic
        hr0 = np.stack([O.shift_and_add(list(x), shifts, F) for x in lr])
    finally:
        O.set_threads(1)
    yy, xx = np.mgrid[0:PN, 0:PN]
    hr0[2] = np.where(((yy // 8 + xx // 8) & 1) == 0, 0.0, 255.0)
    lr.setflags(write=False), hr0.setflags(write=False)
    return lr, hr0


@functools.lru_cache(maxsize=None)
def reference(cfg, n_iter):
    from oracle import sr_oracle as O
    shifts, psf = CFGS[cfg][0], CFGS[cfg][1]()
    lr, hr0 = inputs(cfg)
    O.set_threads(8)
    try:
        res = [O.ibp(list(lr[i]), shifts, psf, hr0[i], F, n_iter, 0.5) for i in range(B)]
    finally:
        O.set_threads(1)
    hr, errs = np.stack([r[0] for r in res]), np.stack([np.asarray(r[1], dtype=np.float64) for r in res])
    hr.setflags(write=False), errs.setflags(write=False)
    return hr, errs


def test_the_clip_patch_clips_on_both_sides_of_the_boundary():
    """the oracle's own result on the third patch: pixels on 0.0 and on 255.0 in the resident rows and in the parked rows of several blocks"""
    for n_iter in (1, 2, 3):
        hr = reference("grid16_gauss", n_iter)[0][2]
        row = np.arange(PN)[:, None] % 64
        for lo, hi in ((0, 16), (16, 64)):
            for bound in (0.0, 255.0):
                hit = (hr == bound) & (row >= lo) & (row < hi)
                blocks = {(y // 64, x // 64) for y, x in zip(*np.nonzero(hit))}
                assert len(blocks) >= 4, (n_iter, lo, hi, bound, sorted(blocks))


@pytest.mark.parametrize("n_iter", [1, 2, 3])
@pytest.mark.parametrize("cfg", sorted(CFGS))
def test_patch_resident_rows_vs_oracle(cfg, n_iter):
    S.set_precision("f32")
    shifts, psf = CFGS[cfg][0], CFGS[cfg][1]()
    lr_h, hr0_h = inputs(cfg)
    hr_o, err_o = reference(cfg, n_iter)
    lr, hr0 = torch.tensor(lr_h, dtype=torch.float32, device="cuda"), torch.tensor(hr0_h, dtype=torch.float32, device="cuda")
    lr_c, hr0_c = lr.clone(), hr0.clone()
    # out of place, the output between guard bands
    g = MG.Guarded.tensor((B, PN, PN), torch.float32, "cuda")
    hr, errs = S.ibp_batched(lr, shifts, psf, hr0, F, n_iter, 0.5, out=g.t)
    assert S.last_path() == "patch" and hr.data_ptr() == g.t.data_ptr()
    g.check("hr_out")
    assert torch.equal(lr, lr_c) and torch.equal(hr0, hr0_c), "an input was written"
    got, got_e = hr.cpu().numpy().astype(np.float64), errs.cpu().numpy()
    for i in range(B):
        d = float(np.abs(got[i] - hr_o[i]).max())
        rel = float(np.abs(got_e[i] / err_o[i] - 1).max())
        print(f"{cfg} n_iter={n_iter} patch {i}: max |hr - oracle| = {d:.3e} DN, max relative trace error = {rel:.3e}")
        assert d <= TOL, (i, d)
        np.testing.assert_allclose(got_e[i], err_o[i], rtol=ERR_RTOL)
        for bound in (0.0, 255.0):
            at = hr_o[i] == bound
            assert np.array_equal(got[i][at], hr_o[i][at]), f"patch {i}: {int((got[i][at] != bound).sum())} of {int(at.sum())} pixels the oracle clips to {bound} are elsewhere"
    # the same call again: the same bits
    hr_r, errs_r = S.ibp_batched(lr, shifts, psf, hr0, F, n_iter, 0.5)
    assert torch.equal(hr_r, hr) and torch.equal(errs_r, errs)
    # hr_out aliasing hr_init, guarded as well
    a = MG.Guarded.tensor((B, PN, PN), torch.float32, "cuda")
    a.t.copy_(hr0)
    hr_a, errs_a = S.ibp_batched(lr, shifts, psf, a.t, F, n_iter, 0.5, out=a.t)
    assert S.last_path() == "patch" and hr_a.data_ptr() == a.t.data_ptr()
    a.check("hr_out == hr_init")
    assert torch.equal(hr_a, hr) and torch.equal(errs_a, errs), "in place: a different state or trace"
    assert torch.equal(lr, lr_c), "the frames were written"
