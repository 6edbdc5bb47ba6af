"""srx_ibp_* off the values the rest of the suite shares: step 0.3 and 1.0 instead of 0.5, 15 ... 32 frames, a random start image, and
frames on which clip(.., 0, 255) acts in every iteration -- every route (patch, stile, ctile, ztile, dtile, atile, mosaic, btile, fused,
composed) against oracle.sr_oracle.ibp (float64) on the cases of tests/offdefaults_cases.py.  tests/test_ibp_offdefaults_host.py checks,
without a GPU, that each case goes to the kernel named here and that the reference puts 2.6 ... 7.2 % of its pixels on each bound.

Per case and precision (test_case): (1) 4 iterations at step 0.3 and 1.0 through the default route, every flagged route and once with the
7 x 7 asymmetric PSF: state within IBP_TOL, trace within ERR_RTOL (test_gpu_parity's own figures).  (2) The clip: 0 <= hr <= 255 exactly,
and where the oracle is exactly 0.0 / 255.0 so is the kernel, except where the oracle's value before the clip lies within the tolerance
of the bound; those exceptions are counted and may be 0.5 % of the clipped pixels (the oracle against itself from a start perturbed by
the tolerance: at most 1 pixel in 1000).  (3) out= aliasing hr_init, a batch of two, the shape-only workspace bound and the uint8 entry
give the bits of the plain call, at step 0.3.  Then a plan in instalments (p->step) and one shift table per item, at step 0.3.

Measured on an MI355X, worst max |gpu - oracle| over the cases of a route (DN):
    float32 (bound 1e-3)   step 0.3   step 1.0   7 x 7 PSF: 0.3 / 1.0
      patch                3.6e-05    3.6e-05    3.5e-05 / 3.7e-05
      ztile                3.3e-05    3.5e-05    3.5e-05 / 3.2e-05
      ctile                3.3e-05    3.3e-05
      dtile                3.7e-05    3.6e-05    3.4e-05 / 3.5e-05
      atile                3.8e-05    3.6e-05
      mosaic               3.6e-05    3.9e-05    3.5e-05 / 3.7e-05
      btile                2.9e-05    3.4e-05    3.1e-05 / 3.0e-05
      fused                3.5e-05    3.6e-05    3.1e-05 / 3.7e-05
      composed             2.8e-05    2.7e-05    2.3e-05 / 2.8e-05
    float64 (bound 1e-8)
      stile                8.5e-14    1.4e-13
      ctile                8.5e-14    1.1e-13
      mosaic               3.1e-13    9.7e-13    1.5e-12 / 4.3e-12
      fused                1.0e-12    2.7e-12    1.4e-12 / 3.5e-12
      composed             2.8e-14    5.7e-14    5.7e-14 / 5.7e-14
MSE trace: at most 2.4e-8 relative in float32 and 1.5e-15 in float64.  No pixel the oracle clips was off its bound in any run, so the
allowance of (2) was never drawn on.  Sensitivity, each change alone in a scratch build: step replaced by 0.5 in k_ibp_ztile's sn fails
the four float32 z_* cases and the plan test; the upper clip bound of k_bwd_mosaic raised to 256 fails all 16 cases that reach the tile
kernels (hr.max() = 256.0); `C <= 16` admitted to k_ztile_pack's packed form fails z_c16 in float32.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import offdefaults_cases as C  # noqa: E402
import sr_mi355x as S  # noqa: E402
from sr_mi355x import api  # noqa: E402
from test_gpu_parity import ERR_RTOL, IBP_TOL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["f64", "f32"])
def prec(request):
    S.set_precision(request.param)
    yield request.param
    S.set_precision("f32")


@pytest.fixture(scope="module", autouse=True)
def release_references():
    """the cached inputs and oracle runs (some tens of MB) go when the module is done: nothing later in the session runs beside them"""
    yield
    C.reference.cache_clear()
    C.inputs.cache_clear()


def dev(a, prec):
    """a fresh device copy (the shared inputs are read-only)"""
    return torch.from_numpy(np.array(a)).to("cuda", torch.float64 if prec == "f64" else torch.float32)


def same(a, b):
    """state bit for bit; the trace as test_batch_equals_loop compares it"""
    return torch.equal(a[0], b[0]) and np.allclose(a[1].cpu().numpy(), b[1].cpu().numpy(), rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("case", sorted(C.CASES))
def test_case(prec, case):
    c = C.CASES[case]
    f, shifts, tol = c["f"], c["shifts"], IBP_TOL[prec]
    lr, init = C.inputs(case)
    lr2, init2 = C.inputs(case, C.SEED + 1)
    lr_b, init_b = dev(np.stack([lr, lr2]), prec), dev(np.stack([init, init2]), prec)
    bad = []
    for psf_name, routes in (("gauss", c["routes"][prec]), ("asym", [(C.AUTO, c["asym"][prec])])):
        psf = C.PSFS[psf_name]()
        for step in C.STEPS:
            ref = C.reference(case, psf_name, step)
            for flags, want in routes:
                hr, errs = S.ibp_batched(lr_b[:1], shifts, psf, init_b[:1], f, C.N_ITER, step, flags=flags)
                assert S.last_path() == want, (psf_name, step, hex(flags), S.last_path())
                hr, errs = hr[0].double().cpu().numpy(), errs[0].cpu().numpy()
                d = float(np.abs(hr - ref["hr"]).max())
                e = float(np.max(np.abs(errs - ref["errors"]) / ref["errors"]))
                clipped, near, far = C.clip_misses(hr, ref, tol)
                tag = f"{case} {prec} {psf_name} step {step} {want}"
                print(f"offdefaults {tag}: max |gpu - oracle| = {d:.3e}, trace rel = {e:.2e}, min {hr.min()!r} max {hr.max()!r}, "
                      f"{clipped} clipped, {near} off the bound within the tolerance, {far} beyond it")
                if not d <= tol:
                    bad.append(f"{tag}: max |gpu - oracle| = {d:.3e} > {tol:.0e}")
                if not e <= ERR_RTOL[prec]:
                    bad.append(f"{tag}: trace off by {e:.2e} > {ERR_RTOL[prec]:.0e}")
                if not (hr.min() >= 0.0 and hr.max() <= 255.0):
                    bad.append(f"{tag}: range {hr.min()!r} .. {hr.max()!r}")
                if far or near > C.CLIP_EXCEPTIONS * clipped:
                    bad.append(f"{tag}: of {clipped} clipped pixels {near} are off the bound within the tolerance and {far} beyond it")
    assert not bad, "\n".join(bad)

    # the forms of the call, at step 0.3 on the default route
    psf, step = C.PSFS["gauss"](), C.STEPS[0]
    want = c["routes"][prec][0][1]
    one = S.ibp_batched(lr_b[:1], shifts, psf, init_b[:1], f, C.N_ITER, step)
    two = S.ibp_batched(lr_b[1:], shifts, psf, init_b[1:], f, C.N_ITER, step)
    assert not torch.equal(one[0], two[0])
    buf = init_b[:1].clone()
    alias = S.ibp_batched(lr_b[:1], shifts, psf, buf, f, C.N_ITER, step, out=buf)
    assert S.last_path() == want and alias[0].data_ptr() == buf.data_ptr()
    assert same(alias, one), "out= aliasing hr_init"
    both = S.ibp_batched(lr_b, shifts, psf, init_b, f, C.N_ITER, step)
    assert S.last_path() == want
    assert same((both[0][:1], both[1][:1]), one) and same((both[0][1:], both[1][1:]), two), "a batch of two against its items"
    bound = S.ibp_batched(lr_b[:1], shifts, psf, init_b[:1], f, C.N_ITER, step, exact_workspace=False)
    assert S.last_path() == want and same(bound, one), "exact_workspace=False"
    u8 = S.ibp_u8_batched(np.array(lr, dtype=np.uint8)[None], shifts, psf, init_b[:1], f, C.N_ITER, step)
    assert S.last_path() == want and same(u8, one), "the uint8 entry"


def test_plan_in_instalments_at_step_0_3():
    """srx_ibp_plan_*: step travels through the plan; 1 + 3 iterations equal the one call bit for bit (z_n17, float32: k_ibp_ztile)"""
    S.set_precision("f32")
    c = C.CASES["z_n17"]
    lr, init = (dev(a[None], "f32") for a in C.inputs("z_n17"))
    psf, step = C.PSFS["gauss"](), C.STEPS[0]
    one, e1 = S.ibp_batched(lr, c["shifts"], psf, init, c["f"], C.N_ITER, step)
    assert S.last_path() == "ztile"
    p = api.IbpPlan(lr, c["shifts"], psf, init, c["f"], step)
    try:
        assert p.path == "ztile"
        parts = [p.run(1), p.run(3)]
        assert torch.equal(p.result(), one) and torch.equal(torch.cat(parts, dim=1), e1)
    finally:
        p.close()
    ref = C.reference("z_n17", "gauss", step)
    assert float(np.abs(one[0].double().cpu().numpy() - ref["hr"]).max()) <= IBP_TOL["f32"]


def test_per_item_tables_at_step_0_3(prec):
    """shifts_yx [B, N, 2] on b_n15's shape: each item of the batch equals its own B = 1 call"""
    c = C.CASES["b_n15"]
    want = c["routes"][prec][0][1]
    psf, step, f = C.PSFS["gauss"](), C.STEPS[0], c["f"]
    lr = dev(np.stack([C.inputs("b_n15")[0], C.inputs("b_n15", C.SEED + 1)[0]]), prec)
    init = dev(np.stack([C.inputs("b_n15")[1], C.inputs("b_n15", C.SEED + 1)[1]]), prec)
    hr, errs = S.ibp_batched(lr, C.PER_ITEM_TABLES, psf, init, f, C.N_ITER, step)
    assert S.last_path() == want
    for b in range(2):
        h1, e1 = S.ibp_batched(lr[b:b + 1], C.PER_ITEM_TABLES[b], psf, init[b:b + 1], f, C.N_ITER, step)
        assert S.last_path() == want
        assert torch.equal(h1[0], hr[b]) and torch.equal(e1[0], errs[b]), b
    assert not torch.equal(hr[0], hr[1])
    ref = C.reference("b_n15", "gauss", step)  # item 0 is the case itself
    assert float(np.abs(hr[0].double().cpu().numpy() - ref["hr"]).max()) <= IBP_TOL[prec]
