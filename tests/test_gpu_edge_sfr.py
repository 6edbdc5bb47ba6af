"""srx_edge_sfr_* / metrics_device.edge_sfr on the GPU, cal_target_report(fused=True) and session.queue_metrics_device built on them.

The inputs are those of tests/test_edge_sfr_host.py (tests/edge_sfr_cases.py): the two golden 200 x 200 ROIs and eight seeded noisy synthetic
edges, each as uint8, float32 and float64.  Two references: sr_mi355x.metrics at the tolerances tests/test_gpu_metrics.py holds the device
composition to, and the host model (tests/edge_sfr_host_model.cpp, the same plain arithmetic compiled with g++), which the device must
equal BIT FOR BIT up to the ESF on integer samples -- every sum is an integer there -- while the trigonometric tail (DFT, atan2: device and
host libm differ in the last place) is held to the tolerances.

The memory-contract cases register their ids through test_gpu_memory_contract.ids (each names its entry point); the outputs of these
entry points are `void *`, so the census of tests/test_memguard_host.py does not ask for them."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import edge_sfr_cases as C
import memguard as MG
import test_gpu_memory_contract as T
from sr_mi355x import _lib, api, metrics as M, metrics_device as D, session

pytestmark = pytest.mark.gpu
CUDA = "cuda"
DT = {"u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}
ROIS = C.rois()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    if C.GXX is None:
        pytest.skip("no g++")
    return C.build_model(str(tmp_path_factory.mktemp("sfr_model") / "edge_sfr_host_model"), sanitize=False)


def dev(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a)).to(CUDA).to(DT[kind])


def items(handle):
    """EdgeSfr -> the dicts of edge_sfr_cases.item, from one copy back"""
    s, e, m, st = (t.cpu().numpy() for t in (handle.summary, handle.esf, handle.mtf, handle.status))
    return [C.item(st[b], s[b], e[b], m[b]) for b in range(handle.B)]


def raw(handle):
    return tuple(t.cpu().numpy().tobytes() for t in (handle.summary, handle.esf, handle.mtf, handle.status))


@pytest.mark.parametrize("side", list(C.SIDES))
@pytest.mark.parametrize("name", list(ROIS))
def test_integer_samples_against_model_and_metrics(model, tmp_path, name, side):
    ref = C.reference(ROIS[name], side, key=name)
    mod = C.run_model(model, tmp_path, ROIS[name], side)
    got = {k: D.edge_sfr(dev(ROIS[name], k), side=side) for k in DT}
    assert raw(got["u8"]) == raw(got["f32"]) == raw(got["f64"])  # the same integers in three element types: the same bits
    it = items(got["u8"])[0]
    C.same_integer_part(it, mod)
    C.close_to_reference(it, ref)
    res = got["f64"].result()  # the wrapper's dict
    assert res["status"] == 0 and res["mtf50"] == it["mtf50"] and res["nbin"] == 72 and len(res["esf_x"]) == 72 and len(res["mtf"]) == 36
    assert np.array_equal(res["esf_y"], it["esf_y"]) and np.array_equal(res["freq"], it["freq"])


def test_non_integer_float64_samples_against_metrics():
    roi = C.edge(37, 53, 0.35, seed=5) * 0.75 + 0.3
    for side in C.SIDES:
        C.close_to_reference(items(D.edge_sfr(dev(roi, "f64"), side=side))[0], C.reference(roi, side))


@pytest.mark.parametrize("kind", list(DT))
def test_batch_items_get_their_single_roi_bits_and_calls_repeat(kind):
    a = np.stack([ROIS["synth_37x53_0.35"], ROIS["synth_37x53_1.25"], C.edge(37, 53, 0.8, seed=9).astype(np.uint8)])
    x = dev(a, kind)
    batch = D.edge_sfr(x)
    b_items = items(batch)
    assert [i["status"] for i in b_items] == [0, 0, 0] and len({i["m"] for i in b_items}) == 3
    for b in range(3):
        one = D.edge_sfr(x[b])
        for t_b, t_1 in zip((batch.summary, batch.esf, batch.mtf, batch.status), (one.summary, one.esf, one.mtf, one.status)):
            assert t_b[b].cpu().numpy().tobytes() == t_1[0].cpu().numpy().tobytes(), b
    assert raw(D.edge_sfr(x)) == raw(batch)  # run to run


@pytest.mark.parametrize("kind", list(DT))
def test_roi_read_in_place_inside_a_stack(kind):
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 256, (3, 96, 131)).astype(np.uint8)
    for b, (h, w, a) in enumerate(((48, 64, 1.2), (48, 64, 0.3), (48, 64, 0.7))):
        frames[b, 5:5 + h, 3:3 + w] = C.edge(h, w, a, seed=40 + b).astype(np.uint8)
    stack = dev(frames, kind)
    before = stack.clone()
    view = stack[:, 5:53, 3:67]
    assert not view.is_contiguous() and view.data_ptr() == stack.data_ptr() + (5 * 131 + 3) * stack.element_size()
    got = D.edge_sfr(view)
    assert got._keep[0].data_ptr() == view.data_ptr()  # nothing was copied
    assert raw(got) == raw(D.edge_sfr(view.contiguous()))
    assert [i["status"] for i in items(got)] == [0, 0, 0] and torch.equal(stack, before)
    assert raw(D.edge_sfr(view[1])) == tuple(t[1:2].cpu().numpy().tobytes() for t in (got.summary, got.esf, got.mtf, got.status))
    with pytest.raises(ValueError):
        D.edge_sfr(stack[:, :, ::2])


def test_esf_and_mtf_are_optional():
    x = dev(ROIS["synth_37x53_0.35"], "u8")
    full = D.edge_sfr(x)
    lib = _lib.load()
    summary, status = torch.full((1, C.SUMMARY), 7.0, dtype=torch.float64, device=CUDA), torch.full((1,), 7, dtype=torch.int32, device=CUDA)
    ws = api._ws(lib.srx_edge_sfr_scratch_bytes(1, 37, 53))
    rc = lib.srx_edge_sfr_u8(T.p(x), 1, 37, 53, 53, 0, 0, 1.5, T.p(summary), None, None, T.p(status), ws[1], ws[2], api._stream())
    assert rc == 0 and torch.equal(summary.view(torch.int64), full.summary.view(torch.int64)) and int(status[0]) == 0


def test_statuses(model, tmp_path):
    const = np.full((37, 53), 9, np.uint8)
    tiny = C.edge(8, 8, 0.3, seed=1)
    for a, kind in ((const, "u8"), (const, "f32"), (tiny, "f64")):
        it = items(D.edge_sfr(dev(a, kind)))[0]
        mod = C.run_model(model, tmp_path, a, "left")
        assert it["status"] == mod["status"] == 1 and it["n_edge"] == mod["n_edge"] < 20 and it["threshold"] == mod["threshold"]
        assert np.isnan(it["esf"]).all() and np.isnan(it["mtf_raw"]).all() and it["zero"] == 0.0
        assert np.array_equal(np.isnan(it["summary"]), np.isnan(mod["summary"]))
        assert all(np.isnan(it[k]) for k in ("mtf50", "mtf10", "angle_deg", "m", "b", "n_side", "nbin", "lo", "hi", "flipped", "m_c", "b_c"))
    res = D.edge_sfr(dev(const, "u8")).result()
    assert res["status"] == 1 and len(res["esf_x"]) == 0 and len(res["mtf"]) == 0
    # a batch with a failing item in the middle: the others are untouched by it
    a = np.stack([ROIS["synth_37x53_0.35"], const, ROIS["synth_37x53_1.25"]])
    got = items(D.edge_sfr(dev(a, "u8")))
    assert [i["status"] for i in got] == [0, 1, 0]
    assert np.array_equal(C.bits(got[2]["summary"]), C.bits(items(D.edge_sfr(dev(a[2], "u8")))[0]["summary"]))


STATUS_CASES = C.status_cases()


@pytest.mark.parametrize("name", list(STATUS_CASES))
def test_statuses_2_and_4_and_short_curves_against_the_model(model, tmp_path, name):
    """thin and small ROIs (edge_sfr_cases.status_cases): no pixel on a side (2, k_sfr_bins returns before it writes), one filled bin of
    four (4, decided in k_sfr_tail, the angle written and esf / mtf NaN), and status 0 with 12 / 13 / 53 bins"""
    a, want = STATUS_CASES[name]
    for side in C.SIDES:
        mod = C.run_model(model, tmp_path, a, side)
        got = [items(D.edge_sfr(dev(a, k), side=side))[0] for k in DT]
        assert all(np.array_equal(C.bits(g["summary"]), C.bits(got[0]["summary"])) and g["status"] == got[0]["status"] for g in got)
        assert got[0]["status"] == mod["status"] == want
        if want == 0:
            C.same_integer_part(got[0], mod)
            nbin = int(got[0]["nbin"])
            assert 4 <= nbin < 72 and (got[0]["esf"][:, nbin:] == 0).all() and (got[0]["mtf_raw"][:, nbin // 2:] == 0).all()
        else:
            C.same_failed_item(got[0], mod)


def test_threshold_zero_between_tied_order_statistics(model, tmp_path):
    z = C.zero_plane()
    mag = C.magnitude(z)
    assert (mag == 0).mean() > 0.85
    for kind in DT:
        it = items(D.edge_sfr(dev(z, kind)))[0]
        assert it["threshold"] == 0.0 and it["n_edge"] == (mag > 0).sum()
        C.close_to_reference(it, C.reference(z, "left", key="zero_plane"))
    C.same_integer_part(it, C.run_model(model, tmp_path, z, "left"))


# =====================================================================================================================================
# memory contract: guards around the four outputs and the workspace, three poisons, intact inputs, an element-aligned img
# =====================================================================================================================================
CONTRACT = {"37x53": np.stack([ROIS["synth_37x53_0.35"], ROIS["synth_37x53_1.25"]]), "200x200": ROIS["golden_SAA"][None]}
CONTRACT_IDS = [f"srx_edge_sfr_{k}-{c}-skip{s}" for k in DT for c in CONTRACT for s in (0, 1)]


@pytest.mark.parametrize("cid", CONTRACT_IDS, ids=T.ids(CONTRACT_IDS))
def test_memory_contract(cid):
    entry, case, skip = cid.split("-")
    kind, skip = entry.rsplit("_", 1)[1], int(skip[4:])
    a = CONTRACT[case]
    B, H, W = a.shape
    x = T.put(dev(a, kind), skip)  # skip = 1: img one element off the 256-byte grid
    assert x.data_ptr() % 256 == skip * x.element_size()
    lib = _lib.load()
    summary, esf = T.out((B, C.SUMMARY), torch.float64), T.out((B, 2, C.MAX_BINS), torch.float64)
    mtf, status = T.out((B, 2, C.MAX_BINS // 2), torch.float64), T.out((B,), torch.int32)
    st = api._stream()

    def call(wp, wn):
        return getattr(lib, entry)(T.p(x), B, H, W, W, H * W, 0, 1.5, T.p(summary.t), T.p(esf.t), T.p(mtf.t), T.p(status.t), wp, wn, st)

    res = T.contract(call, [summary, esf, mtf, status], lib.srx_edge_sfr_scratch_bytes(B, H, W), [x])
    want = D.edge_sfr(x)
    for got, w in zip(res, (want.summary, want.esf, want.mtf, want.status)):
        assert got.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    assert res[3].tolist() == [0] * B


def test_wrapper_refuses_other_inputs():
    with pytest.raises(ValueError):
        D.edge_sfr(np.zeros((40, 40)))
    with pytest.raises(ValueError):
        D.edge_sfr(torch.zeros((2, 2, 40, 40), device=CUDA))
    with pytest.raises(ValueError):
        D.edge_sfr(torch.zeros((40, 40), dtype=torch.int32, device=CUDA))
    with pytest.raises(ValueError):
        D.edge_sfr(torch.zeros((40, 40), device=CUDA), side="top")
    with pytest.raises(_lib.SrxError):
        D.edge_sfr(torch.zeros((1025, 1024), device=CUDA))


# =====================================================================================================================================
# the report and the session hook
# =====================================================================================================================================
def _close(v, w):
    return (np.isnan(v) and np.isnan(w)) or abs(v - w) <= 1e-6 * max(1.0, abs(v))


def test_fused_report_equals_the_composed_one():
    """the synthetic chart of test_gpu_metrics.test_full_frame_psnr_and_report_from_device_images, as float32 and as bytes"""
    f = 2
    H, W = 1536 * f, 2048 * f
    yy, xx = np.mgrid[0:H, 0:W]
    (r0, r1), (c0, c1) = M.ROI2_LR
    cyr, cxr = 0.5 * (r0 + r1) * f, 0.5 * (c0 + c1) * f
    d = ((xx - cxr) * np.cos(0.35) + (yy - cyr) * np.sin(0.35))
    img = 40.0 + 170.0 / (1.0 + np.exp(-(np.abs(d) - 22.0) / 1.6))
    bars = 128.0 + 100.0 * np.sign(np.sin(yy / 3.1))
    c = M.ROI1_COL_LR * f
    img[:, c - 40:c + 40] = bars[:, c - 40:c + 40]
    rng = np.random.default_rng(9)
    q = torch.from_numpy(np.clip(img + rng.normal(0, 1.5, img.shape), 0, 255).astype(np.uint8)).cuda()
    q2 = torch.from_numpy(np.clip(0.97 * img + 3 + rng.normal(0, 1.5, img.shape), 0, 255).astype(np.uint8)).cuda()
    images = {"a": q.float(), "b": q2.float()}
    plain = D.cal_target_report(images, factor=f)
    for fused in (D.cal_target_report(images, factor=f, fused=True), D.cal_target_report({"a": q, "b": q2}, factor=f, fused=True)):
        assert list(fused) == ["a", "b"]
        for title in plain:
            assert set(fused[title]) == set(plain[title])
            for k, v in plain[title].items():
                assert _close(v, fused[title][k]), (title, k, v, fused[title][k])
        assert np.isfinite(plain["a"]["mtf50"]) and np.isnan(plain["b"]["mtf50"])  # (the second chart's curve never falls through: nan both ways)
    with pytest.raises(ValueError):
        D.cal_target_report({"a": q[:100]}, factor=f, fused=True)


def test_queued_metrics_json_equals_the_file_based_report(tmp_path):
    """the session of test_gpu_session.test_metrics_json_from_device_tensors_equals_the_file_based_report with session.queue_metrics_device
    as the hook: after flush_writes() metrics.json is there and equals the notebook summary computed on the host from the PNGs"""
    api.set_precision("f32")
    h, w = 1536, 2048
    yy, xx = np.mgrid[0:h, 0:w]
    (r0, r1), (c0, c1) = M.ROI2_LR
    d = (xx - 0.5 * (c0 + c1)) * np.cos(0.35) + (yy - 0.5 * (r0 + r1)) * np.sin(0.35)
    img = 40.0 + 170.0 / (1.0 + np.exp(-(np.abs(d) - 12.0) / 0.4))
    c = M.ROI1_COL_LR
    img[:, c - 20:c + 20] = (128.0 + 90.0 * np.sign(np.sin(yy / 2.3)))[:, c - 20:c + 20]
    rng = np.random.default_rng(12)
    sess = tmp_path / "data" / "cal_target_full"
    sess.mkdir(parents=True)
    for k, (fname, _) in enumerate(session.IMAGE_SHIFTS):
        Image.fromarray(np.clip(np.roll(img, (k % 2, k // 2), axis=(0, 1)) + rng.normal(0, 1.0, img.shape), 0, 255).astype(np.uint8)).save(sess / fname)
    written = session.process_session(str(sess), api.make_gaussian_psf(), str(tmp_path / "results"), n_iter=5, verbose=False, flush=False,
                                      on_images=session.queue_metrics_device)
    session.flush_writes()
    path = os.path.join(written[0], "metrics.json")
    assert os.path.exists(path) and os.path.exists(os.path.join(written[0], "done.flag"))
    got = json.load(open(path))
    os.rename(path, path + ".queued")
    host = session.write_metrics(written[0])  # from the PNGs, host numpy
    for title in ("native_2x", "SAA", "SAA_IBP"):
        assert set(got[title]) == set(host[title])
        for k, v in host[title].items():
            assert _close(v, got[title][k]), (title, k, v, got[title][k])
        assert np.isfinite(host[title]["mtf50"]) and host[title]["mean_contrast"] > 0.1
    q = {n: np.array(Image.open(os.path.join(written[0], n + ".png"))) for n in ("native_2x", "SAA", "SAA_IBP")}
    for n in ("native_2x", "SAA"):
        assert abs(got["psnr_db"][f"SAA_IBP_vs_{n}"]["affine_fit"] - M.psnr_affine(q[n], q["SAA_IBP"])) < 1e-6
        assert abs(got["psnr_db"][f"SAA_IBP_vs_{n}"]["plain"] - M.psnr(q[n], q["SAA_IBP"])) < 1e-9
