#!/usr/bin/env python3
"""ws_sweep.py -- every workspace query of include/srx.h over a grid of arguments, one line per call: query, arguments, bytes.

Host only (the queries and srx_*_path_for need no device); the library is the one SRX_LIB names, else the package's own.  Two builds size
every workspace alike exactly when their outputs are byte-identical:

    SRX_LIB=/path/to/parent/libsrx.so python3 tools/ws_sweep.py > a.txt
    python3 tools/ws_sweep.py > b.txt && cmp a.txt b.txt

--reduced prints the few hundred lines kept as tests/golden/workspace_bytes.txt (tests/test_workspace_host.py compares the built library
with them); generate that file with the library of the commit BEFORE a change to the workspace code, never with the one under test.

The *_for queries take the shift tables and PSFs of IBP_CASES (tests/test_gpu_memory_contract.py): one case per value of srx_last_path().
The sweep asserts that srx_ibp_path_for met all ten of those names and that no line was skipped.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from sr_mi355x import _lib  # noqa: E402

PATHS = {"patch", "ztile", "ctile", "stile", "dtile", "atile", "mosaic", "btile", "fused", "composed"}
EBS = (4, 8)
# every path-forcing and diagnostic flag that route_ibp / route_saa, the eligible() predicates or a plan() read (one at a time, and the
# one pair the tests use)
FLAGS = (0, _lib.FLAG_COMPOSED, _lib.FLAG_FUSED, _lib.FLAG_PER_FRAME, _lib.FLAG_TILES, _lib.FLAG_TILES | _lib.FLAG_PER_FRAME,
         _lib.FLAG_DIAG_NO_ZERO_FUSE, _lib.FLAG_DIAG_NO_SEPARABLE, _lib.FLAG_DIAG_NO_PREFILTER_TILE, _lib.FLAG_DIAG_V1,
         _lib.FLAG_DIAG_WIDE_WINDOWS, _lib.FLAG_DIAG_COLUMN_TILES, _lib.FLAG_DIAG_TWO_LAUNCH, _lib.FLAG_DIAG_SAA_ONE_PASS,
         _lib.FLAG_DIAG_U8_BYTE_LOADS)

FULL = dict(B=(0, 1, 2, 7, 8, 9, 1024, 32768, 40000), N=(1, 3, 4, 5, 16, 17, 32), f=(1, 2, 3, 4),
            hw=((32, 32), (64, 64), (128, 128), (256, 256), (577, 577), (1536, 2048)), flags=FLAGS, case_hw=None,
            halfwidth=(0, 1, 2, 3, 4, 5, 6, 7, 8), search=(0, 1, 2, 3, 4, 5), nbin=(0, 1, 16, 64), psf_eb=(1, 4, 8))
# (case_hw "own": every case of IBP_CASES at its own shape, batch and flags, so that every path is present)
REDUCED = dict(B=(2, 40000), N=(5,), f=(2, 4), hw=((64, 64), (577, 577)), flags=(0, _lib.FLAG_FUSED, _lib.FLAG_COMPOSED), case_hw="own",
               halfwidth=(1, 7), search=(0, 4), nbin=(1, 64), psf_eb=(1, 8))


def _hd(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return a, a.ctypes.data_as(_lib._HD)


def _cases():
    """(id, f, shifts, psf, (f, shift table, PSF) as a key, own (h, w), own B, own flags, own eb) of every case of IBP_CASES"""
    import test_gpu_memory_contract as T
    out = []
    for c in T.IBP_CASES:
        sh = np.asarray(c["shifts"], dtype=np.float64)
        key = (c["f"], tuple(map(tuple, sh)), c["psf"])
        out.append((T._ibp_id(c), c["f"], sh, np.asarray(T._PSF[c["psf"]], dtype=np.float64), key, c["hw"], c["B"], c["flags"], T.EB[c["prec"]]))
    return out


def sweep(lib, grid):
    """yields the lines; raises if a path of srx_last_path() was not met or a line went missing"""
    n_expected = n = 0
    met = set()

    def line(name, args, value):
        nonlocal n
        n += 1
        return f"{name} {' '.join(f'{k}={v}' for k, v in args)} -> {value}"

    G = grid
    # ---- the primitives
    for eb in EBS:
        for B in G["B"]:
            for (h, w) in G["hw"]:
                n_expected += 3 + len(G["f"])
                a = (("eb", eb), ("B", B), ("H", h), ("W", w))
                yield line("srx_shift_workspace_bytes", a, lib.srx_shift_workspace_bytes(eb, B, h, w))
                yield line("srx_forward_workspace_bytes", a, lib.srx_forward_workspace_bytes(eb, B, h, w))
                yield line("srx_backproject_workspace_bytes", a, lib.srx_backproject_workspace_bytes(eb, B, h, w))
                for f in G["f"]:
                    yield line("srx_zoom_workspace_bytes", a + (("f", f),), lib.srx_zoom_workspace_bytes(eb, B, h, w, f))
    # ---- shape-only shift_and_add / ibp, in every form
    for eb in EBS:
        for B in G["B"]:
            for N in G["N"]:
                for f in G["f"]:
                    for (h, w) in G["hw"]:
                        a = (("eb", eb), ("B", B), ("N", N), ("h", h), ("w", w), ("f", f))
                        n_expected += 3 + 4 * len(G["flags"])
                        for q in ("srx_saa_workspace_bytes", "srx_saa_u8lr_workspace_bytes", "srx_saa_items_workspace_bytes"):
                            yield line(q, a, getattr(lib, q)(eb, B, N, h, w, f))
                        for fl in G["flags"]:
                            for q in ("srx_ibp_workspace_bytes", "srx_ibp_u8lr_workspace_bytes", "srx_ibp_items_workspace_bytes",
                                      "srx_ibp_plan_workspace_bytes"):
                                yield line(q, a + (("flags", hex(fl)),), getattr(lib, q)(eb, B, N, h, w, h * f, w * f, f, fl))
    # ---- with the shift table and the PSF
    seen = set()
    for (cid, f, sh, k, key, own_hw, own_B, own_fl, own_eb) in _cases():
        own = G["case_hw"] == "own"
        if not own and key in seen:
            continue
        seen.add(key)
        N, (kh, kw) = len(sh), k.shape
        _, shp = _hd(sh)
        _, kp = _hd(k)
        for eb in ((own_eb,) if own else EBS):
            for (h, w) in ((own_hw,) if own else G["hw"]):
                for fl in ((own_fl,) if own else G["flags"]):
                    a = (("case", cid), ("eb", eb), ("N", N), ("h", h), ("w", w), ("f", f), ("flags", hex(fl)))
                    n_expected += 2
                    path = lib.srx_ibp_path_for(eb, N, h, w, h * f, w * f, f, shp, kp, kh, kw, fl).decode()
                    met.add(path)
                    yield line("srx_ibp_path_for", a, path)
                    yield line("srx_saa_path_for", a, lib.srx_saa_path_for(eb, N, h, w, f, shp, fl).decode())
                    for B in ((own_B,) if own else G["B"]):
                        ab = a + (("B", B),)
                        n_expected += 4
                        for q in ("srx_ibp_workspace_bytes_for", "srx_ibp_u8lr_workspace_bytes_for"):
                            yield line(q, ab, getattr(lib, q)(eb, B, N, h, w, h * f, w * f, f, shp, kp, kh, kw, fl))
                        # one table per item: every item the case's, then every other item a table of its own
                        tab = np.ascontiguousarray(np.broadcast_to(sh, (max(B, 1), N, 2)))
                        yield line("srx_ibp_items_workspace_bytes_for", ab + (("tables", "equal"),),
                                   lib.srx_ibp_items_workspace_bytes_for(eb, B, N, h, w, h * f, w * f, f, tab.ctypes.data_as(_lib._HD), kp, kh, kw, fl))
                        tab = tab.copy()
                        tab[1::2] += (np.arange(len(tab[1::2]))[:, None, None] % 7 + 1) / 64.0
                        yield line("srx_ibp_items_workspace_bytes_for", ab + (("tables", "alternating"),),
                                   lib.srx_ibp_items_workspace_bytes_for(eb, B, N, h, w, h * f, w * f, f, tab.ctypes.data_as(_lib._HD), kp, kh, kw, fl))
    # ---- metrics, registration, the measured PSF
    for B in G["B"]:
        for (h, w) in G["hw"]:
            for nbin in G["nbin"]:
                n_expected += 1
                yield line("srx_metrics_workspace_bytes", (("B", B), ("H", h), ("W", w), ("nbin", nbin)), lib.srx_metrics_workspace_bytes(B, h, w, nbin))
            for eb in EBS:
                for N in G["N"]:
                    for s in G["search"]:
                        n_expected += 1
                        yield line("srx_register_workspace_bytes", (("eb", eb), ("B", B), ("N", N), ("H", h), ("W", w), ("search", s)),
                                   lib.srx_register_workspace_bytes(eb, B, N, h, w, s))
    for eb in G["psf_eb"]:
        for N in G["N"]:
            for (h, w) in G["hw"]:
                for hwid in G["halfwidth"]:
                    n_expected += 1
                    yield line("srx_psf_estimate_workspace_bytes", (("eb", eb), ("N", N), ("H", h), ("W", w), ("halfwidth", hwid)),
                               lib.srx_psf_estimate_workspace_bytes(eb, N, h, w, hwid))
    assert met >= PATHS, f"the sweep never met {sorted(PATHS - met)}"
    assert n == n_expected, f"{n_expected - n} lines skipped"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reduced", action="store_true", help="the few hundred lines of tests/golden/workspace_bytes.txt")
    args = ap.parse_args()
    n = 0
    for ln in sweep(_lib.load(), REDUCED if args.reduced else FULL):
        print(ln)
        n += 1
    print(f"{n} lines, library {_lib.SO_PATH}", file=sys.stderr)


if __name__ == "__main__":
    main()
