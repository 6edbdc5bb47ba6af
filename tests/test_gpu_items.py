"""One shift table per item of a batch (srx_saa_items_*, srx_ibp_items_*; api.*_batched with shifts_yx [B, N, 2]).

The contract (include/srx.h): item b of an items call returns exactly the bits of the shared-table call with B = 1 on item b's frames,
hr_init and table -- output, MSE trace, hr_out == hr_init.  The reference everywhere is therefore that B = 1 call (held to the oracle by
tests/test_gpu_parity.py), compared with torch.equal.  Shapes: 128 x 160 HR is two windows per axis for both "btile" kernels (152 padded
rows over 96 / 100 owned), the smallest at which a window's row-range decisions differ between windows and items.

The memory-contract cases at the end register their ids with tests/test_gpu_memory_contract.py's list (its ids()), which is what
tests/test_memguard_host.py compares include/srx.h with: the items entry points write device memory and have their cases here."""
import ctypes
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import memguard as MG  # noqa: E402
import sr_mi355x as S  # noqa: E402
import test_gpu_memory_contract as MC  # noqa: E402
from oracle import sr_oracle as O  # noqa: E402
from sr_mi355x import _lib, api, session, synth  # noqa: E402
from test_gpu_parity import ERR_RTOL, IBP_TOL  # noqa: E402

pytestmark = pytest.mark.gpu

EB = {"f32": 4, "f64": 8}
DT = {"f32": torch.float32, "f64": torch.float64}
M4 = np.asarray(synth.MEASURED_4)
N4 = np.asarray(synth.NOMINAL_4)
# (0.62, -0.71): floor(2 s) = 1 / -2 where the other frames have 0 / -1, so tap origins and their ranges differ between frames and items
BTILE_TABLES = np.stack([M4, -M4, np.asarray([(0.62, -0.71), (0.4897, 0.4641), (-0.4798, -0.4553), (-0.4856, 0.4369)])])
LARGE = np.asarray([(2.5, 0.0), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)])  # |f s| > 4: "composed"
PSFS = {"gauss": synth.gaussian_psf, "asym": synth.asymmetric_psf, "full7": synth.full_support_psf}


def jitter(table, seed, amp=0.05):
    return np.asarray(table, dtype=np.float64) + np.random.default_rng(seed).uniform(-amp, amp, np.shape(table))


def path_for(prec, table, psf, h, w, f, flags=0):
    sh = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    k = np.ascontiguousarray(np.asarray(psf, dtype=np.float64))
    return _lib.load().srx_ibp_path_for(EB[prec], len(sh), h, w, h * f, w * f, f, sh.ctypes.data_as(_lib._HD), k.ctypes.data_as(_lib._HD),
                                        k.shape[0], k.shape[1], flags).decode()


def saa_path_for(prec, table, h, w, f, flags=0):
    sh = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    return _lib.load().srx_saa_path_for(EB[prec], len(sh), h, w, f, sh.ctypes.data_as(_lib._HD), flags).decode()


_frames_cache = {}


def frames(B, N, h, w, prec, seed=0):
    """LR frames [B, N, h, w] and a start image [B, 2 h .. ] on the device: smooth scenes plus noise, not integers (computed once per shape)"""
    key = (B, N, h, w, prec, seed)
    if key not in _frames_cache:
        rng = np.random.default_rng(100 + seed)
        base = np.stack([synth.truth_image(h, w, seed=700 + seed + b) for b in range(B)])
        lr = np.clip(base[:, None] + rng.normal(0.0, 6.0, (B, N, h, w)), 0, 255)
        _frames_cache[key] = torch.from_numpy(lr).to("cuda", DT[prec])
    return _frames_cache[key]


def one_by_one(lr, tables, psf, hr0, f, n_iter, prec, flags=0):
    """the reference: the shared-table call with B = 1 on every item -> (hr, errors, names)"""
    hrs, errs, names = [], [], []
    for b in range(lr.shape[0]):
        hr, e = S.ibp_batched(lr[b:b + 1], tables[b], psf, hr0[b:b + 1], f, n_iter, 0.5, precision=prec, flags=flags)
        hrs.append(hr[0]), errs.append(e[0]), names.append(S.last_path())
    return torch.stack(hrs), torch.stack(errs), names


def start_image(lr, tables, f, prec):
    return torch.stack([S.shift_and_add_batched(lr[b:b + 1], tables[b], f, precision=prec)[0] for b in range(lr.shape[0])])


# ---- 1. "btile", one table per item -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("psf_name", sorted(PSFS))
def test_btile_per_item(psf_name):
    prec, f, h, w, n_iter = "f32", 2, 64, 80, 3
    psf, tables = PSFS[psf_name](), BTILE_TABLES
    for t in tables:
        assert path_for(prec, t, psf, h, w, f) == "btile"
    lr = frames(3, 4, h, w, prec)
    hr0 = start_image(lr, tables, f, prec)
    ref_hr, ref_e, names = one_by_one(lr, tables, psf, hr0, f, n_iter, prec)
    assert names == ["btile"] * 3
    hr, e = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec)
    assert S.last_path() == "btile"
    for b in range(3):
        assert torch.equal(hr[b], ref_hr[b]), f"item {b}: max |d| = {float((hr[b] - ref_hr[b]).abs().max())}"
        assert torch.equal(e[b], ref_e[b]), (b, e[b], ref_e[b])
    assert not torch.equal(hr[0], hr[1])
    # the shape-only workspace bound, and the call without a trace
    hr_b, e_b = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec, exact_workspace=False)
    assert torch.equal(hr_b, hr) and torch.equal(e_b, e)
    hr_n, e_n = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec, want_errors=False)
    assert e_n is None and torch.equal(hr_n, hr)
    # hr_out == hr_init
    buf = hr0.clone()
    hr2, e2 = S.ibp_batched(lr, tables, psf, buf, f, n_iter, 0.5, precision=prec, out=buf)
    assert hr2.data_ptr() == buf.data_ptr() and torch.equal(hr2, hr) and torch.equal(e2, e)
    # run to run
    hr3, e3 = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec)
    assert torch.equal(hr3, hr) and torch.equal(e3, e)
    # item 2 against the oracle
    hr_o, err_o = O.ibp(list(lr[2].double().cpu().numpy()), [tuple(s) for s in tables[2]], psf, hr0[2].double().cpu().numpy(), f, n_iter, 0.5)
    d = float(np.abs(hr[2].double().cpu().numpy() - hr_o).max())
    print(f"btile per item [{psf_name}]: item 2 max |gpu - oracle| = {d:.3e}, trace {e[2].cpu().numpy()} / {np.asarray(err_o)}")
    assert d <= IBP_TOL["f32"]
    np.testing.assert_allclose(e[2].cpu().numpy(), err_o, rtol=ERR_RTOL["f32"])


def test_btile_per_item_tables_longer_than_one_upload():
    """An item's table is 4 + 20 N words and one parameter launch carries 960: with N = 4 (84 words) eleven items fit (924) and twelve do
    not (1008), so B = 12 is the smallest batch whose tables go up in two launches, item 11's record split between them.  The smallest
    frame "btile" takes (32 x 32 HR); the per-item contract as above."""
    prec, f, h, w, n_iter, B, N = "f32", 2, 16, 16, 2, 12, 4
    words = 4 + 20 * N
    assert (B - 1) * words <= 960 < B * words
    psf = synth.gaussian_psf()
    tables = np.stack([jitter(M4, 40 + b) for b in range(B)])
    for t in tables:
        assert path_for(prec, t, psf, h, w, f) == "btile"
    lr = frames(B, N, h, w, prec, seed=6)
    hr0 = start_image(lr, tables, f, prec)
    ref_hr, ref_e, names = one_by_one(lr, tables, psf, hr0, f, n_iter, prec)
    assert names == ["btile"] * B
    hr, e = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec)
    assert S.last_path() == "btile"
    for b in range(B):
        assert torch.equal(hr[b], ref_hr[b]), f"item {b}: max |d| = {float((hr[b] - ref_hr[b]).abs().max())}"
        assert torch.equal(e[b], ref_e[b]), (b, e[b], ref_e[b])
    assert not torch.equal(hr[10], hr[11])


# ---- 2. mixed routes --------------------------------------------------------------------------------------------------------------
def test_mixed_routes():
    prec, f, h, w, n_iter = "f32", 2, 64, 80, 3
    psf = synth.gaussian_psf()
    tables = np.stack([N4, jitter(N4, 1), jitter(N4, 2), N4, LARGE])
    want = [path_for(prec, t, psf, h, w, f) for t in tables]
    assert "btile" in want and len(set(want) - {"btile"}) >= 2, want
    lr = frames(5, 4, h, w, prec, seed=1)
    hr0 = start_image(lr, tables, f, prec)
    ref_hr, ref_e, names = one_by_one(lr, tables, psf, hr0, f, n_iter, prec)
    assert names == want
    hr, e = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec)
    assert S.last_path() == "mixed"
    for b in range(5):
        assert torch.equal(hr[b], ref_hr[b]), (b, want[b], float((hr[b] - ref_hr[b]).abs().max()))
        assert torch.equal(e[b], ref_e[b]), (b, want[b])
    buf = hr0.clone()
    hr2, e2 = S.ibp_batched(lr, tables, psf, buf, f, n_iter, 0.5, precision=prec, out=buf)
    assert torch.equal(hr2, hr) and torch.equal(e2, e)


# ---- 3. all tables equal: the shared-table call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["nominal", "measured"])
def test_all_tables_equal(table):
    prec, f, h, w, n_iter = "f32", 2, 64, 80, 3
    psf, t = synth.gaussian_psf(), {"nominal": N4, "measured": M4}[table]
    lr = frames(3, 4, h, w, prec, seed=2)
    hr0 = S.shift_and_add_batched(lr, t, f, precision=prec)
    ref_hr, ref_e = S.ibp_batched(lr, t, psf, hr0, f, n_iter, 0.5, precision=prec)
    name = S.last_path()
    hr, e = S.ibp_batched(lr, np.stack([t] * 3), psf, hr0, f, n_iter, 0.5, precision=prec)
    assert S.last_path() == name
    assert torch.equal(hr, ref_hr) and torch.equal(e, ref_e)


# ---- 4. other precisions and factors ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,f,h,w,B", [("f64", 2, 32, 40, 2), ("f32", 4, 24, 32, 2), ("f32", 3, 24, 32, 2)])
def test_other_precisions_and_factors(prec, f, h, w, B):
    psf, n_iter = synth.gaussian_psf(), 3
    tables = np.stack([jitter(N4, 10 + b) for b in range(B)])
    want = [path_for(prec, t, psf, h, w, f) for t in tables]
    lr = frames(B, 4, h, w, prec, seed=3)
    hr0 = start_image(lr, tables, f, prec)
    ref_hr, ref_e, names = one_by_one(lr, tables, psf, hr0, f, n_iter, prec)
    assert names == want
    hr, e = S.ibp_batched(lr, tables, psf, hr0, f, n_iter, 0.5, precision=prec)
    assert S.last_path() == (want[0] if len(set(want)) == 1 else "mixed")
    for b in range(B):
        assert torch.equal(hr[b], ref_hr[b]) and torch.equal(e[b], ref_e[b]), (b, want[b])


# ---- 5. shift_and_add -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["f32", "f64"])
@pytest.mark.parametrize("f", [2, 4])
def test_shift_and_add_per_item(prec, f):
    h, w = 40, 56
    lr = frames(3, 4, h, w, prec, seed=4)
    for tables, want in ((np.stack([M4, jitter(N4, 20), -M4]), "fused"),           # one per-item run
                         (np.stack([N4, jitter(N4, 21), LARGE]), "mixed"),          # "mosaic", "fused", "composed"
                         (np.stack([jitter(N4, 22), N4, jitter(N4, 23)]), "mixed")):  # two per-item runs of one item round a shared one
        ref = []
        for b in range(3):
            ref.append(S.shift_and_add_batched(lr[b:b + 1], tables[b], f, precision=prec)[0])
        out = S.shift_and_add_batched(lr, tables, f, precision=prec)
        assert S.last_path() == want
        for b in range(3):
            assert torch.equal(out[b], ref[b]), (b, float((out[b] - ref[b]).abs().max()))
    for t in (N4, M4):  # all equal: the shared-table call
        ref = S.shift_and_add_batched(lr, t, f, precision=prec)
        name = S.last_path()
        out = S.shift_and_add_batched(lr, np.stack([t] * 3), f, precision=prec)
        assert S.last_path() == name and torch.equal(out, ref)


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_shift_and_add_routes_match_the_host_query(prec):
    f, h, w = 2, 40, 56
    tables = np.stack([N4, jitter(N4, 21), LARGE])
    lr = frames(3, 4, h, w, prec, seed=4)
    want = [saa_path_for(prec, t, h, w, f) for t in tables]
    assert len(set(want)) == 3, want
    for b in range(3):
        S.shift_and_add_batched(lr[b:b + 1], tables[b], f, precision=prec)
        assert S.last_path() == want[b], b
    S.shift_and_add_batched(lr, tables, f, precision=prec)
    assert S.last_path() == "mixed"


def test_shift_and_add_per_item_run_crosses_the_chunk():
    """2100 items of 16 frames, every table different and on "fused": a chunk is 32768 // 16 = 2048 items, so the batch is walked as
    2048 + 52 (about 350 parameter launches for the 336 000 words of taps)"""
    prec, f, h, w, B, N = "f32", 2, 8, 8, 2100, 16
    tables = np.stack([jitter(synth.phase_shifts(4), 1000 + b) for b in range(B)])
    assert all(not np.array_equal(tables[b], tables[b + 1]) for b in range(B - 1))
    assert {saa_path_for(prec, t, h, w, f) for t in tables} == {"fused"}
    lr = torch.from_numpy(np.random.default_rng(31).uniform(0.0, 255.0, (B, N, h, w))).to("cuda", DT[prec])
    out = S.shift_and_add_batched(lr, tables, f, precision=prec)
    assert S.last_path() == "fused"
    for b in (0, 2047, 2048, 2099):
        ref = S.shift_and_add_batched(lr[b:b + 1], tables[b], f, precision=prec)[0]
        assert torch.equal(out[b], ref), (b, float((out[b] - ref).abs().max()))


def test_uint8_frames_with_per_item_tables():
    f, h, w = 2, 64, 80
    lr8 = frames(3, 4, h, w, "f32", seed=5).round().to(torch.uint8)
    lr = lr8.float()
    psf = synth.gaussian_psf()
    saa8 = S.shift_and_add_u8_batched(lr8, BTILE_TABLES, f, precision="f32")
    saa = S.shift_and_add_batched(lr, BTILE_TABLES, f, precision="f32")
    assert torch.equal(saa8, saa)
    hr8, e8 = S.ibp_u8_batched(lr8, BTILE_TABLES, psf, saa, f, 2, 0.5, precision="f32")
    hr, e = S.ibp_batched(lr, BTILE_TABLES, psf, saa, f, 2, 0.5, precision="f32")
    assert torch.equal(hr8, hr) and torch.equal(e8, e)


# ---- 6. memory contract -----------------------------------------------------------------------------------------------------------
MEM_CASES = {
    "srx_ibp_items_f32-btile_three_tables": ("ibp", "f32", 2, (64, 80), BTILE_TABLES),
    "srx_ibp_items_f32-mixed_routes": ("ibp", "f32", 2, (64, 80), np.stack([N4, jitter(N4, 1), jitter(N4, 2), N4, LARGE])),
    "srx_ibp_items_f64-one_by_one": ("ibp", "f64", 2, (32, 40), np.stack([jitter(N4, 10), jitter(N4, 11)])),
    "srx_saa_items_f32-three_tables": ("saa", "f32", 2, (40, 56), np.stack([M4, jitter(N4, 20), -M4])),
    "srx_saa_items_f64-mixed_routes": ("saa", "f64", 4, (40, 56), np.stack([N4, jitter(N4, 21), LARGE])),
}


def _short_by_a_granule(call, outs, need):
    """contract() refuses need - 1 bytes and a misaligned pointer; this is one whole 256-byte granule short"""
    ws = MG.Guarded(need - 256, "cuda")
    for g in outs:
        g.fill(MG.POISON_GARBAGE)
    st = call(ctypes.c_void_p(ws.ptr), ctypes.c_size_t(need - 256))
    torch.cuda.synchronize()
    assert st == _lib.E_WORKSPACE, st
    ws.check("workspace one granule short")
    assert ws.untouched() and all(g.untouched() for g in outs)
    for i, g in enumerate(outs):
        g.check(f"workspace one granule short: output {i}")


@pytest.mark.parametrize("case", MC.ids(MEM_CASES))
def test_memory_contract(case):
    kind, prec, f, (h, w), tables = MEM_CASES[case]
    B, N = tables.shape[:2]
    L, eb, dt = _lib.load(), EB[prec], DT[prec]
    sh, shp = MC.hd(tables)
    x = MC.put(frames(B, N, h, w, prec, seed=6))
    if kind == "saa":
        o = MC.out((B, h * f, w * f), dt)
        need = L.srx_saa_items_workspace_bytes(eb, B, N, h, w, f)
        call = lambda wp, wn: MC.fn("srx_saa_items", prec)(MC.p(x), B, N, h, w, shp, f, MC.p(o.t), wp, wn, api._stream(), 0)  # noqa: E731
        res = MC.contract(call, [o], need, [x])
        _short_by_a_granule(call, [o], need)
        MC.same(res[0], S.shift_and_add_batched(x, tables, f, precision=prec), case)
        return
    k, kp = MC.hd(synth.gaussian_psf())
    n_iter = 2
    h0 = MC.put(S.shift_and_add_batched(x, tables, f, precision=prec))
    o, e = MC.out((B, h * f, w * f), dt), MC.out((B, n_iter), torch.float64)
    need = L.srx_ibp_items_workspace_bytes_for(eb, B, N, h, w, h * f, w * f, f, shp, kp, 7, 7, 0)
    call = lambda wp, wn: MC.fn("srx_ibp_items", prec)(MC.p(x), B, N, h, w, shp, kp, 7, 7, MC.p(h0), h * f, w * f, f, n_iter, 0.5, MC.p(o.t),  # noqa: E731
                                                      MC.p(e.t), wp, wn, api._stream(), 0)
    res = MC.contract(call, [o, e], need, [x, h0])
    _short_by_a_granule(call, [o, e], need)
    hr, errs = S.ibp_batched(x, tables, k, h0, f, n_iter, 0.5, precision=prec)
    MC.same(res[0], hr, case), MC.same(res[1], errs, case)


# ---- 7. session: process_session(register=True) on a barcode kind, reps batched or one by one ---------------------------------------
def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_session_register_batches_the_reps(tmp_path, monkeypatch):
    from PIL import Image
    table = np.asarray(session.CORNER_SHIFTS, dtype=np.float64)
    sess = tmp_path / "data" / "barcodes"
    sess.mkdir(parents=True)
    for rep in range(2):
        true = table + np.random.default_rng(10 + rep).uniform(-0.15, 0.15, table.shape)
        truth = synth.truth_image(256, 288, seed=5 + rep)
        lr = np.stack([O.forward_model(truth, synth.gaussian_psf(), s, 2) for s in true])
        lr = lr + np.random.default_rng(rep).normal(0.0, 1.0, lr.shape)
        for c, fr in enumerate(np.clip(np.rint(lr), 0, 255).astype(np.uint8)):
            Image.fromarray(fr).save(sess / f"corner{c}_rep{rep:02d}.png")
    psf = synth.gaussian_psf()
    calls = []
    real = api.ibp_batched

    def counted(lr, shifts_yx, *a, **kw):
        calls.append(np.asarray(shifts_yx).shape)
        return real(lr, shifts_yx, *a, **kw)

    monkeypatch.setattr(api, "ibp_batched", counted)
    S.set_precision("f32")
    one = session.process_session(str(sess), psf, str(tmp_path / "batched"), kind="mono_barcodes", n_iter=3, verbose=False, register=True,
                                  batch_reps=True)
    assert calls == [(2, 4, 2)], calls
    del calls[:]
    two = session.process_session(str(sess), psf, str(tmp_path / "looped"), kind="mono_barcodes", n_iter=3, verbose=False, register=True,
                                  batch_reps=False)
    assert calls == [(4, 2), (4, 2)], calls
    assert [os.path.basename(d) for d in one] == [os.path.basename(d) for d in two] == ["rep0", "rep1"]
    for a, b in zip(one, two):
        fa, fb = _files(a), _files(b)
        assert set(fa) == set(fb) and "registration.json" in fa
        for n in fa:
            assert fa[n] == fb[n], f"{os.path.basename(a)}/{n} differs between the batched and the looped run"
    r0, r1 = (json.load(open(os.path.join(d, "registration.json"))) for d in one)
    assert r0["used"] != r1["used"]  # the reps did reconstruct under different tables
