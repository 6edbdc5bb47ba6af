"""The census of the stream-contract test, without a GPU: every prototype of include/srx.h that takes an srx_stream_t is named by a case
id of tests/stream_contract_cases.py (so a new entry point fails here until it has a case, and so does a case that leaves the table),
every srx_ibp case routes to the path it names, and the checker's census rules (tests/streamcheck.py, judge) say what they should."""
import os
import re

import numpy as np

import stream_contract_cases as C
import streamcheck as SC
from sr_mi355x import _lib


# prims: 5 primitives x 2 types, decimate (3 types) and zero_insert (2) at f = 2 and 3, mean_frames / u8_to / quantize_u8 x 2, interleave4,
#   mean_u8 at f = 1, 2 x 2 output types.  saa: 4 routes x 2, the uint8 form on 2 x 2, per-item tables x 2.  ibp: the 14 (path, precision)
#   pairs, 3 uint8 routes, 3 per-item batches, n_iter = 0.  metrics: pair / contrast / rings / spot x 2, magnitude, range, bins x 2, ssim 2 x 2,
#   edge_sfr x 3.  register_psf: 2 x 2 and 3.  png_crc: deflate and file x 3, crc32.  patches: gather x 3, blend x 2.
CASES_PER_FAMILY = {"prims": 31, "saa": 14, "ibp": 21, "plan": 3, "metrics": 19, "register_psf": 7, "png_crc": 7, "patches": 5}


def stream_functions():
    """names of the srx.h prototypes with an srx_stream_t parameter (parsed as test_memguard_host.device_output_functions parses them)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "srx.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return [m.group(1) for m in re.finditer(r"\bint\s+(srx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
            if re.search(r"\bsrx_stream_t\s+\w+", m.group(2))]


def missing(parsed, ids):
    return [n for n in parsed if not any(n in i.split("-") for i in ids)]


def test_every_stream_taking_entry_point_has_a_stream_contract_case():
    parsed = stream_functions()
    assert len(parsed) >= 70 and {"srx_ibp_plan_run", "srx_crc32", "srx_edge_dist_range"} <= set(parsed)
    assert set(parsed) <= set(_lib.symbols())
    ids = list(C.CASES)
    assert not missing(parsed, ids), f"no stream-contract case in tests/stream_contract_cases.py names {missing(parsed, ids)}"
    assert missing(parsed + ["srx_new_entry_f32"], ids) == ["srx_new_entry_f32"]
    # ... and no case leaves the table unnoticed, also where an entry point has several (routes, flags, shapes): the cases per family
    assert {f: len(C.family_ids(f)) for f in C.FAMILIES} == CASES_PER_FAMILY
    assert set(C.FAMILIES) == {c.family for c in C.CASES.values()}


def test_every_ibp_case_routes_to_the_path_it_names():
    """asked of the library's own router (srx_ibp_path_for: host arithmetic, no device), per item for the per-item tables"""
    L, wrong, n = _lib.load(), [], 0
    for c in C.CASES.values():
        assert c.routes or c.family != "ibp" or "mixed" in c.id, c.id
        for prec, sh, psf, (h, w), f, flags, path in c.routes:
            sh = np.ascontiguousarray(sh)
            k = np.ascontiguousarray(np.asarray(C.T._PSF[psf], dtype=np.float64))
            got = L.srx_ibp_path_for({"f32": 4, "f64": 8}[prec], len(sh), h, w, h * f, w * f, f, sh.ctypes.data_as(_lib._HD),
                                     k.ctypes.data_as(_lib._HD), k.shape[0], k.shape[1], flags).decode()
            n += 1
            if got != path:
                wrong.append((c.id, got, path))
    assert not wrong, wrong
    pairs = {(c["path"], c["prec"]) for c in C.first_per_pair()}
    assert len(pairs) == 14 and n >= 14 + 3 + 12
    # the mixed batch: a "btile" run and at least two other routes
    k = np.ascontiguousarray(C.T._PSF["gauss"])
    want = [L.srx_ibp_path_for(4, 4, 64, 80, 128, 160, 2, np.ascontiguousarray(t).ctypes.data_as(_lib._HD), k.ctypes.data_as(_lib._HD), 7, 7, 0).decode()
            for t in C.MIXED_TABLES]
    assert "btile" in want and len(set(want) - {"btile"}) >= 2, want
    # the shift_and_add cases name the route the library reports
    for name in C.SAA_NAMES:
        _, _, f, shifts, (h, w), flags, path, _ = C.T.SAA_CASES[name]
        sh = np.ascontiguousarray(np.asarray(shifts, dtype=np.float64))
        assert L.srx_saa_path_for(4, len(sh), h, w, f, sh.ctypes.data_as(_lib._HD), flags).decode() == path


def test_the_documented_counts_are_the_headers():
    """the numbers the table asserts, found in the text of include/srx.h next to their entry points"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "srx.h")).read().split())
    words = {1: "one kernel launch", 2: "Two kernel launches", 3: "Three kernel launches", 5: "Five kernel launches", 6: "Six kernel launches"}
    for c in C.CASES.values():
        if isinstance(c.kernels, int) and c.kernels > 0:
            assert words[c.kernels].lower() in text.lower(), c.id
    assert "At most three kernel launches" in text and "ceil(n (4 + 20 N) / 960) parameter launches" in text
    assert "two launches per iteration" in text and "three launches per iteration" in text and "8 queued operations / iteration" in text


def test_the_census_rules():
    K, M = SC.KERNEL, SC.MEMCPY
    assert SC.judge([K, K, K], [], kernels=3, copies=0) == []
    assert SC.judge([K, M], ["DtoD"], kernels=None, copies=None) == [] and SC.judge([K, M], [None], copies=None) == []
    assert any("memset node" in s for s in SC.judge([K, SC.MEMSET], [], kernels=1))
    assert any("host node" in s for s in SC.judge([SC.HOST], []))
    assert any("mem-alloc node" in s for s in SC.judge([SC.MEMALLOC, K], []))
    assert any("not device-to-device" in s for s in SC.judge([K, M], ["HtoD"], copies=None))
    assert any("memcpy node(s) where 0 are allowed" in s for s in SC.judge([K, M], ["DtoD"], copies=0))
    assert any("documents 3" in s for s in SC.judge([K, K], [], kernels=3))
    assert any("at most 3" in s for s in SC.judge([K] * 4, [], kernels=("max", 3))) and SC.judge([K] * 2, [], kernels=("max", 3)) == []
    a = np.arange(6.0).reshape(3, 2)
    b = SC.permuted(a)
    assert b.shape == a.shape and sorted(b.ravel()) == sorted(a.ravel()) and not np.array_equal(a, b)
