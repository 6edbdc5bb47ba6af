"""Static checks that go with blk::transpose64's wide LDS reads, on the shipped library's disassembly; no GPU needed.

The transposes of k_ibp_patch read their LDS image sixteen bytes at a time: the rank-1 instantiations must hold no ds_read2_b64 (what
hipcc makes of two adjacent 8-byte reads when the rows are only 8-byte aligned; it runs at the 4-byte rate) and exactly the ds_read_b128
count the source implies.  The form that was measured against this one exchanges half-waves by v_permlane32_swap first, which brings a
hazard of its own -- a VALU write of a swap operand less than two wait states before the swap: tools/isa_lint.py rule H3, checked here
on hand-written listings (the library is held to an empty lint by tests/test_isa_hazards.py)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_lint  # noqa: E402

from sr_mi355x import _lib  # noqa: E402

needs_toolchain = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(os.path.join(isa_lint.LLVM_BIN, "llvm-objdump"))),
                                     reason="ROCm toolchain not installed")

# k_ibp_patch holds two transposes (one per direction of an iteration), each of two passes of 32 add-TID stores and sixteen 16-byte
# reads per lane (one half-wave per pass); the other eight ds_read_b128 are the 16-byte LDS reads the kernel had before the transposes
# read that wide.
T64_PER_KERNEL = 2
READS_B128 = T64_PER_KERNEL * 2 * 16 + 8


def test_lint_recognises_a_write_too_close_to_a_lane_swap():
    bad = """
k:
\tv_mov_b32_e32 v1, v9
\tv_permlane32_swap_b32_e32 v1, v2
\tv_add_f32_e32 v4, v9, v8
\ts_nop 0
\tv_permlane32_swap_b32_e32 v3, v4
\tv_mov_b32_e32 v7, v8
\tv_permlane16_swap_b32_e32 v4, v5
"""
    found = isa_lint.lint(bad)
    assert [f[0] for f in found] == ["H3", "H3", "H3"]
    assert [f[2] for f in found] == [3, 5, 7]  # the line of the write: the v_mov, the v_add one wait state early, the first swap's own write of v4
    good = """
k:
\tv_add_f32_e32 v2, v9, v8
\ts_nop 1
\tv_permlane32_swap_b32_e32 v1, v2
\tv_mov_b32_e32 v4, 0
\tv_mov_b32_e32 v5, 0
\tv_permlane32_swap_b32_e32 v1, v6
\tds_read_b32 v8, v0
\tv_permlane32_swap_b32_e32 v8, v9
\tv_mov_b32_e32 v10, 0
k2:
\tv_permlane32_swap_b32_e32 v10, v11
"""
    assert isa_lint.lint(good) == []


@pytest.fixture(scope="module")
def shipped():
    _lib.build()
    return isa_lint.instructions(isa_lint.disassemble_library(_lib.SO_PATH))


def _by_function(ins, pred):
    out = {}
    for fn, _, mn, _ in ins:
        if pred(fn):
            key = mn[:-4] if mn.endswith(("_e32", "_e64")) else mn  # objdump and -S name the encoding, hand-written listings need not
            out.setdefault(fn, {}).setdefault(key, 0)
            out[fn][key] += 1
    return out


@needs_toolchain
def test_rank1_patch_kernels_read_the_transpose_image_16_bytes_wide(shipped):
    # k_ibp_patch<C01, M8, 0>: the mangled name ends its template arguments with Li0E
    kernels = _by_function(shipped, lambda fn: "k_ibp_patch" in fn and "Li0EEE" in fn)
    assert len(kernels) == 4, sorted(kernels)
    for fn, c in kernels.items():
        assert c.get("ds_read2_b64", 0) == 0, (fn, c.get("ds_read2_b64"))
        assert c.get("ds_read_b128", 0) == READS_B128, (fn, c.get("ds_read_b128"))
        assert c.get("ds_write_addtid_b32", 0) == T64_PER_KERNEL * 64, (fn, c.get("ds_write_addtid_b32"))
