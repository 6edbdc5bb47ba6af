"""The case table of the stream-contract test (tests/streamcheck.py is the checker, tests/stream_contract_worker.py runs a family in a
process of its own, tests/test_gpu_stream_contract.py starts the workers, tests/test_stream_contract_host.py compares the ids with
include/srx.h).  One case per entry point and element type at the small shapes of tests/test_gpu_memory_contract.py, whose helpers
build the calls; a case id names every entry point it calls, joined with "-".  Importing this module needs no device: a case holds a
builder that allocates when the worker calls it.

Kernel-node counts.  `kernels` is what include/srx.h documents for the entry point (an int, or ("max", n)); None where the header gives no
number -- the count observed on an MI355X then stands in the comment above the cases and is not asserted (the census still demands the
same node list from a second capture on other samples).  `diffs` are counts the header gives per iteration or per parameter launch, read
off as the difference between two captures that are counted and never launched.  `copies`: 0 where the header says "no memset or copy
node" or "one kernel launch", None (any number, each device-to-device) elsewhere."""
import ctypes

import numpy as np
import torch

import streamcheck as SC
import test_gpu_memory_contract as T
from sr_mi355x import _lib, metrics, synth
import patchwise_cases as PC

CUDA = "cuda"
U8 = torch.uint8
FAMILIES = ("prims", "saa", "ibp", "plan", "metrics", "register_psf", "png_crc", "patches")
CASES = {}  # id -> Case, in table order


class Case:
    def __init__(self, cid, family, make, kernels=None, copies=None, exact_copies=None, diffs=(), routes=()):
        self.id, self.family, self.make, self.kernels, self.copies, self.exact_copies = cid, family, make, kernels, copies, exact_copies
        self.diffs, self.routes = list(diffs), list(routes)
        assert cid not in CASES, cid
        CASES[cid] = self


def family_ids(family):
    return [c.id for c in CASES.values() if c.family == family]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def last_path():
    return T.lib().srx_last_path().decode()


def out(shape, dtype):
    return torch.empty(tuple(int(s) for s in shape), dtype=dtype, device=CUDA)


def ws(nbytes):
    """(tensor or None, pointer, size): the workspace of exactly the queried size (torch allocations sit on the 256-byte grid)"""
    nbytes = int(nbytes)
    if nbytes == 0:
        return None, None, ctypes.c_size_t(0)
    t = torch.empty(nbytes, dtype=U8, device=CUDA)
    assert t.data_ptr() % 256 == 0
    return t, T.p(t), ctypes.c_size_t(nbytes)


def fsets(shape, prec, seed, integer=True, offset=0.0):
    """three sample sets of a float input: as the memory-contract case draws them, another draw, and one that is not integer-valued"""
    return [T.rnd(shape, prec, seed, integer) + offset, T.rnd(shape, prec, seed + 1000, integer) + offset, T.rnd(shape, prec, seed + 2000, integer=False) + offset]


def u8sets(shape, seed):
    return [T._u8(shape, seed + 1000 * k) for k in range(3)]


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(CUDA, dtype)


def inputs(*sets):
    """-> (device input tensors, samples(k)) for per-input lists of three sample sets"""
    return [torch.empty_like(s[0]) for s in sets], (lambda k: [s[k] for s in sets])


def hd(a):
    """host float64 array -> (a COPY kept alive, pointer): the checker overwrites a case's host arrays in place, and T.hd hands back the
    caller's own array where that is float64 already (the PSFs of T._PSF)"""
    a = np.array(a, dtype=np.float64, order="C", copy=True)
    return a, a.ctypes.data_as(_lib._HD)


def sp(stream):
    return None if stream is None else ctypes.c_void_p(stream)


def jitter(table, seed, amp=0.05):
    return np.asarray(table, dtype=np.float64) + np.random.default_rng(seed).uniform(-amp, amp, np.shape(table))


# ==================================================================================================================================
# prims
# ==================================================================================================================================
PRIM_SHAPE = "B1_37x50_k7x7"


def _prim(func, prec):
    def make():
        B, (H, W), psf, (sy, sx), f, _ = T.PRIM_SHAPES[PRIM_SHAPE]
        dt, eb, L, fn = T.DT[prec], T.EB[prec], T.lib(), T.fn(func, prec)
        k, kp = hd(psf)
        kh, kw = k.shape
        oh, ow = -(-H // f), -(-W // f)
        if func == "srx_backproject":
            (x,), samples = inputs(fsets((B, oh, ow), prec, 12, offset=-128.0))
        else:
            (x,), samples = inputs(fsets((B, H, W), prec, 11))
        if func == "srx_blur":
            o = out((B, H, W), dt)
            return SC.Inst(lambda s: fn(T.p(x), B, H, W, kp, kh, kw, T.p(o), sp(s)), [x], samples, [o], host=[k])
        if func == "srx_shift_cubic":
            o = out((B, H, W), dt)
            w, wp, wn = ws(L.srx_shift_workspace_bytes(eb, B, H, W))
            return SC.Inst(lambda s: fn(T.p(x), B, H, W, sy, sx, T.p(o), wp, wn, sp(s)), [x], samples, [o], w)
        if func == "srx_zoom_cubic":
            o = out((B, H * 2, W * 2), dt)
            w, wp, wn = ws(L.srx_zoom_workspace_bytes(eb, B, H, W, 2))
            return SC.Inst(lambda s: fn(T.p(x), B, H, W, 2, T.p(o), wp, wn, sp(s)), [x], samples, [o], w)
        if func == "srx_forward":
            o = out((B, oh, ow), dt)
            w, wp, wn = ws(L.srx_forward_workspace_bytes(eb, B, H, W))
            return SC.Inst(lambda s: fn(T.p(x), B, H, W, kp, kh, kw, sy / f, sx / f, f, T.p(o), wp, wn, sp(s)), [x], samples, [o], w, host=[k])
        o = out((B, H, W), dt)
        w, wp, wn = ws(L.srx_backproject_workspace_bytes(eb, B, H, W))
        return SC.Inst(lambda s: fn(T.p(x), B, oh, ow, kp, kh, kw, sy / f, sx / f, f, H, W, T.p(o), wp, wn, sp(s)), [x], samples, [o], w, host=[k])
    return make


# observed (kernel nodes, f32 and f64 alike, no copy node): blur 1, shift_cubic 6, zoom_cubic 6, forward 7, backproject 8
for _f in T.PRIM_FUNCS:
    for _pr in T.PRECS:
        Case(f"{_f}_{_pr}-{PRIM_SHAPE}", "prims", _prim(_f, _pr))

IM_H, IM_W, IM_B = 41, 57, 2


def _index_map(func, kind, f=None):
    """kind: "f32" / "f64" / "u8" (srx_decimate_u8) / None (srx_interleave4_u8)"""
    def make():
        L = T.lib()
        dt = T.DT.get(kind, U8)
        fn = getattr(L, f"{func}_{kind}") if kind else getattr(L, func)
        B, H, W, n = IM_B, IM_H, IM_W, IM_H * IM_W
        if func == "srx_decimate":
            py, px = 1, f - 1
            (x,), samples = inputs(u8sets((B, H, W), 51) if kind == "u8" else fsets((B, H, W), kind, 51))
            o = out((B, -(-(H - py) // f), -(-(W - px) // f)), dt)
            return SC.Inst(lambda s: fn(T.p(x), B, H, W, f, py, px, T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_zero_insert":
            eh, ew = -(-H // f), -(-W // f)
            (x,), samples = inputs(fsets((B, eh, ew), kind, 52))
            o = out((B, H, W), dt)
            return SC.Inst(lambda s: fn(T.p(x), B, eh, ew, f, H, W, T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_mean_frames":
            R = 3
            (x,), samples = inputs(fsets((B, R, n), kind, 53, integer=False))
            o = out((B, n), dt)
            return SC.Inst(lambda s: fn(T.p(x), B, R, ctypes.c_size_t(n), T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_u8_to":
            (x,), samples = inputs(u8sets((n,), 54))
            o = out((n,), dt)
            return SC.Inst(lambda s: fn(T.p(x), ctypes.c_size_t(n), T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_quantize_u8":
            (x,), samples = inputs([t * 1.2 - 20 for t in fsets((n,), kind, 55, integer=False)])
            o = out((n,), U8)
            return SC.Inst(lambda s: fn(T.p(x), ctypes.c_size_t(n), T.p(o), sp(s)), [x], samples, [o])
        h, w = 9, 11
        (x,), samples = inputs(u8sets((B, 4, h, w), 56))
        o = out((B, 2 * h, 2 * w), U8)
        return SC.Inst(lambda s: fn(T.p(x), B, h, w, T.p(o), sp(s)), [x], samples, [o])
    return make


# observed: one kernel node each, no copy node
for _f in (2, 3):
    for _k in ("f32", "f64", "u8"):
        Case(f"srx_decimate_{_k}-41x57_f{_f}", "prims", _index_map("srx_decimate", _k, _f))
    for _k in T.PRECS:
        Case(f"srx_zero_insert_{_k}-41x57_f{_f}", "prims", _index_map("srx_zero_insert", _k, _f))
for _func in ("srx_mean_frames", "srx_u8_to", "srx_quantize_u8"):
    for _k in T.PRECS:
        Case(f"{_func}_{_k}-41x57", "prims", _index_map(_func, _k))
Case("srx_interleave4_u8-9x11", "prims", _index_map("srx_interleave4_u8", None))


def _mean_u8(prec, f):
    def make():
        B, R, H, W = 2, 3, 33, 47
        py, px = (0, 0) if f == 1 else (1, 0)
        (x,), samples = inputs(u8sets((B, R, H, W), 57))
        o = out((B, -(-(H - py) // f), -(-(W - px) // f)), T.DT[prec])
        return SC.Inst(lambda s: T.lib().srx_mean_u8(T.p(x), B, R, H, W, f, py, px, T.EB[prec], T.p(o), sp(s)), [x], samples, [o])
    return make


for _pr in T.PRECS:
    for _f in (1, 2):
        Case(f"srx_mean_u8-{_pr}-R3_33x47_f{_f}", "prims", _mean_u8(_pr, _f), kernels=1, copies=0)


# ==================================================================================================================================
# shift_and_add
# ==================================================================================================================================
SAA_NAMES = ("two_pass_x3", "one_pass_x3", "per_frame", "below_the_fused_minimum")
SAA_ITEM_TABLES = np.stack([np.asarray(synth.MEASURED_4), -np.asarray(synth.MEASURED_4)])


def _saa(entry, prec, case):
    def make():
        _, B, f, shifts, (h, w), flags, path, _ = T.SAA_CASES[case]
        N, eb, L, fn = len(shifts), T.EB[prec], T.lib(), T.fn(entry, prec)
        sh, shp = hd(shifts)
        if entry == "srx_saa_u8lr":
            (x,), samples = inputs(u8sets((B, N, h, w), 21))
            need = L.srx_saa_u8lr_workspace_bytes(eb, B, N, h, w, f)
        else:
            (x,), samples = inputs(fsets((B, N, h, w), prec, 21, integer=(case != "per_frame")))
            need = L.srx_saa_workspace_bytes(eb, B, N, h, w, f)
        o = out((B, h * f, w * f), T.DT[prec])
        wt, wp, wn = ws(need)
        return SC.Inst(lambda s: fn(T.p(x), B, N, h, w, shp, f, T.p(o), wp, wn, sp(s), flags), [x], samples, [o], wt, host=[sh], path=path)
    return make


def _saa_items(prec):
    def make():
        B, N, f, (h, w) = 2, 4, 2, (45, 61)
        eb, L, fn = T.EB[prec], T.lib(), T.fn("srx_saa_items", prec)
        sh, shp = hd(SAA_ITEM_TABLES)
        (x,), samples = inputs(fsets((B, N, h, w), prec, 22))
        o = out((B, h * f, w * f), T.DT[prec])
        wt, wp, wn = ws(L.srx_saa_items_workspace_bytes(eb, B, N, h, w, f))
        return SC.Inst(lambda s: fn(T.p(x), B, N, h, w, shp, f, T.p(o), wp, wn, sp(s), 0), [x], samples, [o], wt, host=[sh], path="fused")
    return make


# observed (kernel + memcpy nodes, f32 / f64): two_pass_x3 5 + 0, one_pass_x3 4 + 0, per_frame 14 + 2 / 15 + 1, below_the_fused_minimum 26 + 0;
# the uint8 form: two_pass_x3 5 + 0, per_frame 15 + 2 / 16 + 1 (the conversion of the staged frames); two per-item tables 15 + 2 / 16 + 1
for _c in SAA_NAMES:
    for _pr in T.PRECS:
        Case(f"srx_saa_{_pr}-{_c}", "saa", _saa("srx_saa", _pr, _c))
for _c in ("two_pass_x3", "per_frame"):
    for _pr in T.PRECS:
        Case(f"srx_saa_u8lr_{_pr}-{_c}", "saa", _saa("srx_saa_u8lr", _pr, _c))
for _pr in T.PRECS:
    Case(f"srx_saa_items_{_pr}-two_tables", "saa", _saa_items(_pr))


# ==================================================================================================================================
# ibp
# ==================================================================================================================================
PER_ITERATION = {"patch": 0, "ztile": 1, "ctile": 1, "dtile": 1, "stile": 2, "btile": 2, "atile": 3}  # srx.h, srx_last_path()
# SRX_FLAG_DIAG_V1 (srx.h): 8 queued operations per iteration -- (kernel nodes, memcpy nodes) = 8, 0 in float64, where both prefilters are
# a row and a column kernel; 6, 2 in float32 on planes of at least 64 x 64, where each is the tile kernel and the copy back from its scratch
V1_PER_ITERATION = {"f64": (8, 0), "f32": (6, 2)}


def first_per_pair():
    """the first entry of T.IBP_CASES for every (path, precision) pair"""
    seen, res = set(), []
    for c in T.IBP_CASES:
        if (c["path"], c["prec"]) not in seen:
            seen.add((c["path"], c["prec"]))
            res.append(c)
    return res


def _ibp(entry, c, tables=None, path=None, check_path=True):
    """entry: srx_ibp / srx_ibp_u8lr / srx_ibp_items (then `tables` [B, N, 2], or a function n -> tables).  make(n_iter, flags_or, n)"""
    def make(n_iter=None, flags_or=0, n=None):
        prec, f, (h, w) = c["prec"], c["f"], c["hw"]
        n_it = c["n_iter"] if n_iter is None else n_iter
        flags = c["flags"] | flags_or
        dt, eb, L, fn = T.DT[prec], T.EB[prec], T.lib(), T.fn(entry, prec)
        tb = tables(n) if callable(tables) else tables
        B = c["B"] if tb is None else len(tb)
        sh, shp = hd(c["shifts"] if tb is None else tb)
        N, H, W = sh.shape[-2], h * f, w * f
        k, kp = hd(T._PSF[c["psf"]])
        kh, kw = k.shape
        need = getattr(L, entry + "_workspace_bytes_for")(eb, B, N, h, w, H, W, f, shp, kp, kh, kw, flags)
        assert need > 0, (entry, c["name"], "the library refuses these arguments")
        lr_sets = u8sets((B, N, h, w), 31) if entry == "srx_ibp_u8lr" else fsets((B, N, h, w), prec, 31, c["integer"])
        (lr, init), samples = inputs(lr_sets, fsets((B, H, W), prec, 32, integer=False))
        hr = out((B, H, W), dt)
        errs = out((B, n_it), torch.float64) if n_it > 0 else None   # out of place, with the MSE trace
        wt, wp, wn = ws(need)
        call = lambda s: fn(T.p(lr), B, N, h, w, shp, kp, kh, kw, T.p(init), H, W, f, n_it, 0.5, T.p(hr), T.p(errs), wp, wn, sp(s), flags)  # noqa: E731
        return SC.Inst(call, [lr, init], samples, [hr] + ([errs] if errs is not None else []), wt, host=[sh, k], path=(path or c["path"]) if check_path else None)
    return make


def _route(c, shifts=None, path=None, flags_or=0):
    return (c["prec"], np.asarray(c["shifts"] if shifts is None else shifts, dtype=np.float64), c["psf"], c["hw"], c["f"], c["flags"] | flags_or, path or c["path"])


def _iter_diffs(c):
    d = [(dict(n_iter=3), dict(n_iter=2), PER_ITERATION.get(c["path"]))]
    if c["path"] == "fused":
        d.append((dict(n_iter=3, flags_or=_lib.FLAG_DIAG_V1), dict(n_iter=2, flags_or=_lib.FLAG_DIAG_V1), V1_PER_ITERATION[c["prec"]]))
    return d


# observed at each case's n_iter (kernel nodes; no copy node unless said), and per added iteration where srx.h gives no number:
#   patch 13 (n_iter 3), stile 17, ctile 18 (f64 and f32), ztile 18, dtile 17, atile 16, btile 7;
#   mosaic 10 (+2 per iteration, f32 and f64), fused 9 (+3), composed f32 85 and 13 copies (+36), composed f64 97 and 1 copy (+42);
#   uint8 frames: patch 12, btile 8 (one conversion kernel more), stile 17; per-item: btile B = 12 8, fused f64 two tables 18,
#   the mixed batch of five 154 and 17 copies
for _c in first_per_pair():
    Case(T._ibp_id(_c), "ibp", _ibp("srx_ibp", _c), diffs=_iter_diffs(_c),
         routes=[_route(_c)] + ([_route(_c, path="fused", flags_or=_lib.FLAG_DIAG_V1)] if _c["path"] == "fused" else []))


def _named(path, name, prec="f32"):
    return next(c for c in T.IBP_CASES if c["path"] == path and c["name"] == name and c["prec"] == prec)


# one route that reads the bytes itself and one that stages them; float64 (the strips read the bytes themselves) so that both symbols have a case
for _c in (_named("patch", "x4_grid"), _named("btile", "smallest"), _named("stile", "x4_grid", "f64")):
    Case(f"srx_ibp_u8lr_{_c['prec']}-{_c['path']}-{_c['name']}", "ibp", _ibp("srx_ibp_u8lr", _c), diffs=_iter_diffs(_c)[:1], routes=[_route(_c)])

# a "btile" run of 12 items with N = 4 and pairwise different tables: an item's table is 4 + 20 N = 84 words and a parameter launch carries
# 960, so eleven items go up in one launch and twelve in two (tests/test_gpu_items.py)
ITEMS_BTILE = T._ibp_case("B12_N4_16x16", "btile", "f32", 2, synth.MEASURED_4, (16, 16), n_iter=2)
ITEMS_F64 = T._ibp_case("two_tables_45x61", "fused", "f64", 2, synth.MEASURED_4, (45, 61), n_iter=2)
ITEMS_MIXED = T._ibp_case("five_items_64x80", "mixed", "f32", 2, synth.NOMINAL_4, (64, 80), n_iter=2)
_N4 = np.asarray(synth.NOMINAL_4)
MIXED_TABLES = np.stack([_N4, jitter(_N4, 1), jitter(_N4, 2), _N4, np.asarray([(2.5, 0.0), (0.5, 0.5), (-0.5, -0.5), (-0.5, 0.5)])])


def btile_tables(n=None):
    return np.stack([jitter(synth.MEASURED_4, 40 + b) for b in range(n or 12)])


Case("srx_ibp_items_f32-btile-B12_N4_16x16", "ibp", _ibp("srx_ibp_items", ITEMS_BTILE, btile_tables), diffs=[(dict(n=12), dict(n=11), 1)],
     routes=[_route(ITEMS_BTILE, t) for t in btile_tables()])
Case("srx_ibp_items_f64-fused-two_tables_45x61", "ibp", _ibp("srx_ibp_items", ITEMS_F64, SAA_ITEM_TABLES),
     routes=[_route(ITEMS_F64, t) for t in SAA_ITEM_TABLES])
Case("srx_ibp_items_f32-mixed-five_items_64x80", "ibp", _ibp("srx_ibp_items", ITEMS_MIXED, MIXED_TABLES))
# n_iter = 0 out of place: the state is copied and nothing else happens
Case("srx_ibp_f32-patch-x4_grid-n_iter0", "ibp", lambda: _ibp("srx_ibp", _named("patch", "x4_grid"), check_path=False)(n_iter=0), kernels=0, exact_copies=1,
     routes=[_route(_named("patch", "x4_grid"))])


# ==================================================================================================================================
# plans: create, run(2), get_rows, set_rows, run(1), get_rows(0, H) in ONE capture; destroyed after the launches
# ==================================================================================================================================
def _plan(name):
    def make():
        prec, f, shifts, (h, w), psf, B, path = T.PLAN_CASES[name]
        dt, eb, L = T.DT[prec], T.EB[prec], T.lib()
        N, H, W = len(shifts), h * f, w * f
        sh, shp = hd(shifts)
        k, kp = hd(T._PSF[psf])
        kh, kw = k.shape
        lo, hi = H // 3, H // 3 + 5
        create, get_rows, set_rows = T.fn("srx_ibp_plan_create", prec), T.fn("srx_ibp_plan_get_rows", prec), T.fn("srx_ibp_plan_set_rows", prec)
        (lr, init, rows_in), samples = inputs(fsets((B, N, h, w), prec, 41), fsets((B, H, W), prec, 42, integer=False),
                                              fsets((B, hi - lo, W), prec, 43, integer=False))
        e1, e2 = out((B, 2), torch.float64), out((B, 1), torch.float64)
        mid, full = out((B, hi - lo, W), dt), out((B, H, W), dt)
        wt, wp, wn = ws(L.srx_ibp_plan_workspace_bytes(eb, B, N, h, w, H, W, f, 0))
        plans = []

        def call(s):
            st, h_ = sp(s), ctypes.c_void_p()
            rc = create(T.p(lr), B, N, h, w, shp, kp, kh, kw, T.p(init), H, W, f, 0.5, 0, H, wp, wn, st, 0, ctypes.byref(h_))
            if rc != _lib.OK:
                return rc
            plans.append(h_)
            for step in (lambda: L.srx_ibp_plan_run(h_, 2, T.p(e1), st), lambda: get_rows(h_, lo, hi, T.p(mid), st),
                         lambda: set_rows(h_, lo, hi, T.p(rows_in), st), lambda: L.srx_ibp_plan_run(h_, 1, T.p(e2), st),
                         lambda: get_rows(h_, 0, H, T.p(full), st)):
                rc = step()
                if rc != _lib.OK:
                    return rc
            return _lib.OK

        def cleanup():
            while plans:
                L.srx_ibp_plan_destroy(plans.pop())

        inst = SC.Inst(call, [lr, init, rows_in], samples, [e1, mid, e2, full], wt, host=[sh, k], path=path, cleanup=cleanup)
        inst.get_path = lambda: L.srx_ibp_plan_path(plans[-1]).decode()
        return inst
    return make


# observed for the whole sequence (kernel + memcpy nodes): ztile_hoisted 22 + 0, call_per_run_atile 32 + 1, call_per_run_ctile 38 + 1
for _n in ("ztile_hoisted", "call_per_run_atile", "call_per_run_ctile"):   # (the last: the float64 symbols)
    Case(T._plan_id(_n), "plan", _plan(_n))


# ==================================================================================================================================
# metrics
# ==================================================================================================================================
MH, MW = 61, 97   # the smallest shape of tests/test_gpu_ssim.py


def _pairs(prec, B, seed):
    """three sample sets of (ref, test) [B, MH, MW]; the third not integer-valued"""
    sets = [T._pair((MH, MW), prec, B, seed=seed + 100 * k) for k in range(3)]
    sets[2] = tuple(x * 0.75 + 0.3 for x in sets[2])
    return [s[0] for s in sets], [s[1] for s in sets]


def _metric(func, prec, **kw):
    def make():
        L, H, W = T.lib(), MH, MW
        fn = T.fn(func, prec) if prec else getattr(L, func)
        f64 = torch.float64
        if func == "srx_pair_moments":
            B = 2
            (a, b), samples = inputs(*_pairs(prec, B, 3))
            o = out((B, 7), f64)
            wt, wp, wn = ws(L.srx_metrics_workspace_bytes(B, H, W, 1))
            return SC.Inst(lambda s: fn(T.p(a), T.p(b), B, H, W, 3, T.p(o), wp, wn, sp(s)), [a, b], samples, [o], wt)
        if func == "srx_local_contrast":
            B, n, window = 3, 97, 20
            (x,), samples = inputs(fsets((B, n), prec, 61, integer=False))
            o = out((B, n), T.DT[prec])
            return SC.Inst(lambda s: fn(T.p(x), B, n, window, T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_edge_dist_range":
            m, b = 0.1, 0.45 * W
            o = out((2,), f64)
            return SC.Inst(lambda s: fn(H, W, m, b, float(np.sqrt(1 + m * m)), 1, T.p(o), sp(s)), [], lambda k: [], [o])
        if func == "srx_ssim":
            B, radius, border = 2, 3, 3
            h, w = H - 2 * border, W - 2 * border
            rad, taps, dr = metrics.ssim_params((h, w), np.float64, None, 255.0, True, 0.9)   # Gaussian taps: distinct entries
            assert rad == radius
            taps, tp = hd(taps)
            sets = list(_pairs(prec, B, 5))
            if kw["affine"]:
                sets.append([dev(np.array([[1.0 + 0.01 * k, 0.9 + 0.05 * i, 4.0 - i - k] for i in range(B)]), f64) for k in range(3)])
            ins, samples = inputs(*sets)
            a, b, aff = ins[0], ins[1], (ins[2] if kw["affine"] else None)
            m, smap = out((B,), f64), (out((B, h, w), T.DT[prec]) if kw["map"] else None)
            wt, wp, wn = ws(L.srx_metrics_workspace_bytes(B, H, W, 1))
            call = lambda s: fn(T.p(a), T.p(b), B, H, W, border, radius, tp, 1, dr, 0.01, 0.03, T.p(aff), T.p(m), T.p(smap), wp, wn, sp(s))  # noqa: E731
            return SC.Inst(call, ins, samples, [m] + ([smap] if smap is not None else []), wt, host=[taps])
        # one image [MH, MW]
        if func in ("srx_edge_magnitude_f64", "srx_edge_bins"):
            dt = T.DT[prec] if prec else f64
            rng = np.random.default_rng(71)
            rois = [T._edge_roi(H, W) + rng.integers(-3, 4, (H, W)), np.flipud(T._edge_roi(H, W)) + rng.integers(-3, 4, (H, W)),
                    T._edge_roi(H, W) * 0.75 + 0.3 + rng.uniform(-2, 2, (H, W))]
            (x,), samples = inputs([dev(r, dt) for r in rois])
        else:
            (x,), samples = inputs([T._pair((H, W), prec, seed=7 + 100 * k)[0] * (0.75 if k == 2 else 1.0) + (0.3 if k == 2 else 0.0) for k in range(3)])
        if func == "srx_ring_sums":
            cy, cx = 0.5 * H - 0.25, 0.5 * W + 1.5
            nbin = int(min(cy, cx, H - cy, W - cx))
            o = out((2 * nbin,), f64)
            wt, wp, wn = ws(L.srx_metrics_workspace_bytes(1, H, W, nbin))
            return SC.Inst(lambda s: fn(T.p(x), H, W, cy, cx, nbin, T.p(o), wp, wn, sp(s)), [x], samples, [o], wt)
        if func == "srx_spot_moments":
            o = out((4,), f64)
            return SC.Inst(lambda s: fn(T.p(x), H, W, T.p(o), sp(s)), [x], samples, [o])
        if func == "srx_edge_magnitude_f64":
            o = out((H, W), f64)
            wt, wp, wn = ws(L.srx_metrics_workspace_bytes(1, H, W, 1))
            return SC.Inst(lambda s: fn(T.p(x), H, W, 1.5, T.p(o), wp, wn, sp(s)), [x], samples, [o], wt)
        assert func == "srx_edge_bins"
        m, b, nbin = 0.1, 0.45 * W, 72
        o = out((2 * nbin,), f64)
        wt, wp, wn = ws(L.srx_metrics_workspace_bytes(1, H, W, nbin))
        return SC.Inst(lambda s: fn(T.p(x), H, W, m, b, float(np.sqrt(1 + m * m)), 1, -8.0, 0.25, nbin, T.p(o), wp, wn, sp(s)), [x], samples, [o], wt)
    return make


# observed (kernel nodes, no copy node): pair_moments 2, local_contrast 1, ring_sums 2, spot_moments 1, edge_magnitude 3, edge_dist_range 1,
# edge_bins 2, ssim 2 (with and without affine / map)
for _func in ("srx_pair_moments", "srx_local_contrast", "srx_ring_sums", "srx_spot_moments"):
    for _pr in T.PRECS:
        Case(f"{_func}_{_pr}-61x97", "metrics", _metric(_func, _pr))
Case("srx_edge_magnitude_f64-61x97", "metrics", _metric("srx_edge_magnitude_f64", None))
Case("srx_edge_dist_range-61x97", "metrics", _metric("srx_edge_dist_range", None))
for _pr in T.PRECS:
    Case(f"srx_edge_bins_{_pr}-61x97", "metrics", _metric("srx_edge_bins", _pr))
    Case(f"srx_ssim_{_pr}-61x97_map_affine", "metrics", _metric("srx_ssim", _pr, affine=True, map=True))
    Case(f"srx_ssim_{_pr}-61x97_mean_only", "metrics", _metric("srx_ssim", _pr, affine=False, map=False))

SFR_H, SFR_W, SFR_STACK, SFR_AT = 37, 53, (2, 50, 70), (5, 9)   # the 37 x 53 ROI of tests/test_gpu_edge_sfr.py inside a [B, 50, 70] stack


def _sfr_stack(k, kind):
    B, Hf, Wf = SFR_STACK
    rng = np.random.default_rng(81 + k)
    r, c = np.mgrid[:Hf, :Wf].astype(np.float64)
    items = []
    for b in range(B):
        d = c - (0.10 + 0.03 * k + 0.02 * b) * r - (0.42 + 0.03 * k) * Wf
        img = 40.0 + 170.0 / (1.0 + np.exp(-d / (1.2 + 0.2 * b))) + rng.uniform(-2, 2, (Hf, Wf))
        items.append(img if (k == 2 and kind != "u8") else np.round(img))
    return dev(np.stack(items), T.DT.get(kind, U8))


def _sfr(kind):
    def make():
        L, (B, Hf, Wf), H, W = T.lib(), SFR_STACK, SFR_H, SFR_W
        fn = getattr(L, f"srx_edge_sfr_{kind}")
        (x,), samples = inputs([_sfr_stack(k, kind) for k in range(3)])
        img = ctypes.c_void_p(x.data_ptr() + (SFR_AT[0] * Wf + SFR_AT[1]) * x.element_size())
        summary, esf, mtf, status = out((B, 16), torch.float64), out((B, 2, 80), torch.float64), out((B, 2, 40), torch.float64), out((B,), torch.int32)
        wt, wp, wn = ws(L.srx_edge_sfr_scratch_bytes(B, H, W))
        call = lambda s: fn(img, B, H, W, ctypes.c_size_t(Wf), ctypes.c_size_t(Hf * Wf), 0, 1.5, T.p(summary), T.p(esf), T.p(mtf), T.p(status), wp, wn, sp(s))  # noqa: E731
        return SC.Inst(call, [x], samples, [summary, esf, mtf, status], wt)
    return make


for _k in ("u8", "f32", "f64"):
    Case(f"srx_edge_sfr_{_k}-37x53_in_a_stack", "metrics", _sfr(_k), kernels=6, copies=0)


# ==================================================================================================================================
# registration and the measured PSF
# ==================================================================================================================================
REG_INIT = [(0.0, 0.0), (1.0, 0.0), (0.0, -1.0)]


def _reg_frames(k, kind):
    B, N, H, W = 2, 3, 48, 56
    base = synth.truth_image(H + 8, W + 8, seed=13 + k)
    fr = np.stack([np.stack([base[4 + dy + b:4 + dy + b + H, 4 + dx:4 + dx + W] for dy, dx in ((0, 0), (1, 0), (0, -1))]) for b in range(B)])
    fr = 0.6 * fr + 0.4 * np.roll(fr, 1, axis=3)   # integer offsets plus half a pixel of blur along x
    return dev(fr if (k == 2 and kind != "u8") else np.round(fr), T.DT.get(kind, U8))


def _register(entry, prec):
    def make():
        B, N, H, W, search, border, n_iter, tol = 2, 3, 48, 56, 2, 1, 4, 1e-4
        L, fn = T.lib(), T.fn(entry, prec)
        kind = "u8" if entry == "srx_register_u8" else prec
        (x,), samples = inputs([_reg_frames(k, kind) for k in range(3)])
        init, ip = hd(REG_INIT)
        sh, sc, stt = out((B, N, 2), torch.float64), out((B, N), torch.float64), out((B, N), torch.int32)
        wt, wp, wn = ws(L.srx_register_workspace_bytes(T.EB[prec], B, N, H, W, search))
        call = lambda s: fn(T.p(x), B, N, H, W, 0, ip, search, border, n_iter, tol, T.p(sh), T.p(sc), T.p(stt), wp, wn, sp(s))  # noqa: E731
        return SC.Inst(call, [x], samples, [sh, sc, stt], wt, host=[init])
    return make


# observed: 15 kernel nodes, no copy node, for all four
for _e in ("srx_register", "srx_register_u8"):
    for _pr in T.PRECS:
        Case(f"{_e}_{_pr}-B2_N3_48x56_search2_init", "register_psf", _register(_e, _pr))

PSF_PEAKS = [[(20, 22), (18, 25), (4, 20)], [(15, 30), (28, 12), (20, 40)], [(22, 20), (3, 14), (19, 27)]]   # one frame dropped per set (reach 9)


def _pinholes(k, kind):
    N, H, W = 3, 40, 44
    rng = np.random.default_rng(91 + k)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    fr = np.stack([12.0 + (200.0 - 10 * i) * np.exp(-((yy - py) ** 2 / 3.1 + (xx - px) ** 2 / 2.3)) + rng.uniform(0, 4, (H, W)) for i, (py, px) in enumerate(PSF_PEAKS[k])])
    return dev(fr if (k == 2 and kind != "u8") else np.round(fr), T.DT.get(kind, U8))


def _psf(kind):
    def make():
        N, H, W, hw = 3, 40, 44, 3
        L = T.lib()
        fn = getattr(L, f"srx_psf_estimate_{kind}")
        (x,), samples = inputs([_pinholes(k, kind) for k in range(3)])
        psf, info = out((2 * hw + 1, 2 * hw + 1), torch.float64), out((N, 3), torch.int32)
        wt, wp, wn = ws(L.srx_psf_estimate_workspace_bytes({"u8": 1, "f32": 4, "f64": 8}[kind], N, H, W, hw))
        return SC.Inst(lambda s: fn(T.p(x), N, H, W, hw, T.p(psf), T.p(info), wp, wn, sp(s)), [x], samples, [psf, info], wt)
    return make


for _k in ("u8", "f32", "f64"):
    Case(f"srx_psf_estimate_{_k}-N3_40x44_hw3_one_dropped", "register_psf", _psf(_k), kernels=("max", 3))


# ==================================================================================================================================
# PNG streams, PNG files, CRC-32
# ==================================================================================================================================
PNG_B, PNG_H, PNG_W = 2, 70, 1000


def _png_images(k, kind):
    """one compressible image and one random one; sets 1 and 2 swap which item compresses, so lengths[b] changes between capture and launch"""
    rng = np.random.default_rng(101 + k)
    yy, xx = np.mgrid[:PNG_H, :PNG_W].astype(np.float64)
    smooth = np.floor(30.0 + 3 * k + 0.2 * xx + 0.5 * yy) % 256
    noise = rng.integers(0, 256, (PNG_H, PNG_W)).astype(np.float64)
    imgs = np.stack([smooth, noise] if k == 0 else [noise, smooth])
    if k == 2 and kind != "u8":
        imgs = imgs * 1.1 - 10.3   # fractions and samples outside [0, 255]: the float forms quantise as they read
    return dev(imgs, T.DT.get(kind, U8))


def _slots(outs):
    """the documented-written part: lengths, and bytes [0, lengths[b]) of every slot (a length nobody wrote -- poison -- is clamped to the
    slot: the comparison of `lengths` itself reports it)"""
    slots, lengths = outs
    n = [min(max(int(v), 0), slots.shape[1]) for v in lengths.cpu()]
    return [lengths] + [slots[b, :n[b]] for b in range(len(n))]


def _png(entry, kind):
    def make():
        L, B, H, W = T.lib(), PNG_B, PNG_H, PNG_W
        fn = getattr(L, f"{entry}_{kind}")
        bound, need = (L.srx_png_file_bound(H, W), L.srx_png_file_scratch_bytes(B, H, W)) if entry == "srx_png_file" else (
            L.srx_png_stream_bound(H, W), L.srx_png_scratch_bytes(B, H, W))
        (x,), samples = inputs([_png_images(k, kind) for k in range(3)])
        slots, lengths = out((B, bound), U8), out((B,), torch.int64)
        wt, wp, wn = ws(need)
        return SC.Inst(lambda s: fn(T.p(x), B, H, W, T.p(slots), T.p(lengths), wp, wn, sp(s)), [x], samples, [slots, lengths], wt, written=_slots)
    return make


for _k in ("u8", "f32", "f64"):
    Case(f"srx_png_deflate_{_k}-B2_70x1000", "png_crc", _png("srx_png_deflate", _k), kernels=3, copies=0)
    Case(f"srx_png_file_{_k}-B2_70x1000", "png_crc", _png("srx_png_file", _k), kernels=5, copies=0)

CRC_B, CRC_STRIDE, CRC_MAX = 3, 40001, 40000   # an odd stride: items 1 and 2 start on odd / even byte addresses
CRC_LENGTHS = [[40000, 16385, 1], [63, 40000, 16384], [0, 33333, 40000]]


def _crc():
    L, B = T.lib(), CRC_B
    ins, samples = inputs(u8sets((B * CRC_STRIDE,), 111), [dev(np.asarray(v, dtype=np.int64), torch.int64) for v in CRC_LENGTHS])
    data, lengths = ins
    crc = out((B,), torch.int32)
    wt, wp, wn = ws(L.srx_crc32_scratch_bytes(B, CRC_MAX))
    call = lambda s: L.srx_crc32(T.p(data), B, ctypes.c_size_t(CRC_STRIDE), ctypes.c_size_t(CRC_MAX), T.p(lengths), 0x35AF061E, T.p(crc), wp, wn, sp(s))  # noqa: E731
    return SC.Inst(call, ins, samples, [crc], wt)


Case("srx_crc32-B3_device_lengths_odd_stride", "png_crc", _crc, kernels=2, copies=0)


# ==================================================================================================================================
# patches: tests/patchwise_cases.py's smallest case with more than one patch on each axis and a batch (3 x 4 patches per image)
# ==================================================================================================================================
PATCH_CASE = "B2_70x83"


def _gather(kind):
    def make():
        B, h, w, ph, pw, sy, sx, _ = PC.BLEND_CASES[PATCH_CASE]
        N, P = 3, PC.count(h, ph, sy) * PC.count(w, pw, sx)
        fn = getattr(T.lib(), f"srx_patches_gather_{kind}")
        (x,), samples = inputs(u8sets((B, N, h, w), 121) if kind == "u8" else fsets((B, N, h, w), kind, 121))
        o = out((B * P, N, ph, pw), T.DT.get(kind, U8))
        return SC.Inst(lambda s: fn(T.p(x), B, N, h, w, ph, pw, sy, sx, T.p(o), sp(s)), [x], samples, [o])
    return make


def _blend(prec):
    def make():
        B, H, W, PH, PW, SY, SX, margin = PC.BLEND_CASES[PATCH_CASE]
        fn = T.fn("srx_patches_blend", prec)
        (x,), samples = inputs([dev(PC.random_patches(B, H, W, PH, PW, SY, SX, np.float64, 131 + k), T.DT[prec]) for k in range(3)])
        o = out((B, H, W), T.DT[prec])
        return SC.Inst(lambda s: fn(T.p(x), B, H, W, PH, PW, SY, SX, margin, T.p(o), sp(s)), [x], samples, [o])
    return make


for _k in ("u8", "f32", "f64"):
    Case(f"srx_patches_gather_{_k}-{PATCH_CASE}", "patches", _gather(_k), kernels=1, copies=0)
for _pr in T.PRECS:
    Case(f"srx_patches_blend_{_pr}-{PATCH_CASE}", "patches", _blend(_pr), kernels=1, copies=0)


# ==================================================================================================================================
# the checker checked: stand-in callees (torch ops and plain HIP calls; none of them faults)
# ==================================================================================================================================
def _standin(kind):
    def make():
        (x,), samples = inputs(fsets((64, 33), "f32", 141))
        o, o2 = out((64, 33), torch.float32), out((64, 33), torch.float32)
        other = torch.cuda.Stream()
        h = SC.hip()
        table = torch.arange(64 * 33 // 2, dtype=torch.float64).pin_memory().numpy()   # page-locked host memory, as many bytes as o2

        def call(s):
            if kind == "other_stream":     # the work goes to a stream of the callee's own: it runs, nothing is captured
                with torch.cuda.stream(other):
                    torch.mul(x, 2.0, out=o)
                    torch.add(x, 1.0, out=o2)
                return 0
            torch.mul(x, SCALAR[0] if kind == "host_scalar" else 2.0, out=o)   # (the current stream is the one the checker passes)
            if kind == "host_scalar":      # a parameter that differs from call to call: the launch repeats what the capture saw
                SCALAR[0] += 0.5
            if kind == "memset":
                return h.hipMemsetAsync(T.p(o2), 0, o2.numel() * 4, sp(s))
            if kind == "host_copy":        # a table uploaded with a host copy: the launch reads the host array as it is THEN
                return h.hipMemcpyAsync(T.p(o2), ctypes.c_void_p(table.ctypes.data), o2.numel() * 4, 1, sp(s))
            return h.hipMemcpyAsync(T.p(o2), T.p(o), o.numel() * 4, 3, sp(s))   # a device-to-device copy: allowed
        return SC.Inst(call, [x], samples, [o, o2], host=[table] if kind == "host_copy" else [])
    return make


SCALAR = [2.0]
SELFTEST = {"standin-sound": (_standin("sound"), None), "standin-other_stream": (_standin("other_stream"), "written during the capture"),
            "standin-memset": (_standin("memset"), "memset node"), "standin-host_scalar": (_standin("host_scalar"), "differs from the plain call"),
            "standin-host_copy": (_standin("host_copy"), "differs from the plain call")}
