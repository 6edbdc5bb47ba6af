"""The checker checked (tests/memguard.py on CPU tensors): planted faults -- a byte stored in front of / behind a payload, an output element
nobody wrote, a workspace byte copied into a result before anything wrote it, a modified input -- are each reported, with the right
offset; a well-behaved call passes; the payload is 256-byte aligned and exactly as long as asked.  And the list of entry points the GPU
memory-contract tests declare covers every function of include/srx.h that takes a device output pointer."""
import os
import re

import pytest
import torch

import memguard as MG

CPU = "cpu"


@pytest.mark.parametrize("n", [1, 255, 256, 257, (1 << 20) + 3])
def test_payload_is_aligned_and_exact(n):
    g = MG.Guarded(n, CPU)
    assert g.ptr % 256 == 0 and g.payload.numel() == n and g.nbytes == n
    assert g.front.numel() >= MG.GUARD_BYTES and g.back.numel() >= MG.GUARD_BYTES
    assert g.back.data_ptr() == g.ptr + n  # the byte behind the payload is guard
    assert g.front.data_ptr() + g.front.numel() == g.ptr
    assert g.damage() is None and g.untouched()
    i = torch.arange(1000, dtype=torch.int64)
    assert torch.equal(g.back[:1000], ((131 * i + 7) & 0xFF).to(torch.uint8))  # position dependent: no constant run matches it
    assert len(set(g.back[:256].tolist())) == 256


def test_typed_views_and_element_aligned_tensors():
    g = MG.Guarded.tensor((3, 5), torch.float64, CPU)
    assert g.t.shape == (3, 5) and g.t.dtype == torch.float64 and g.t.data_ptr() == g.ptr and g.nbytes == 120
    assert bool(torch.isnan(g.t).all())  # POISON_NAN
    g.fill(MG.POISON_GARBAGE)
    assert bool(torch.isfinite(g.t).all()) and float(g.t.abs().min()) > 1e50
    f = MG.Guarded.tensor((7,), torch.float32, CPU, poison=MG.POISON_GARBAGE)
    assert abs(float(f.t[0]) - 1.3e7) < 1e6
    i32 = MG.Guarded.tensor((2,), torch.int32, CPU)
    assert i32.t.tolist() == [-1, -1]
    s = MG.Guarded.tensor((3, 5), torch.float32, CPU, skip=1)
    assert s.t.data_ptr() == s.ptr + 4 and s.nbytes == 64 and s.t.data_ptr() + 60 == s.back.data_ptr()
    s.t.zero_()
    s.check()
    s.payload[0] = 0  # the slack in front of an element-aligned tensor is not the call's to write
    with pytest.raises(AssertionError, match="slack"):
        s.check()
    w = MG.Guarded(1024, CPU)
    assert w.view(torch.float32, (4, 8)).data_ptr() == w.ptr


def _buffers():
    out = MG.Guarded.tensor((4, 6), torch.float32, CPU)
    ws = MG.Guarded(512, CPU)
    x = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    return out, ws, x


def _good(out, ws, x):
    scratch = ws.view(torch.float32, (4, 6))
    scratch.copy_(x * 2)       # writes its scratch before reading it
    out.t.copy_(scratch + 1)
    return 0


def test_a_well_behaved_call_passes():
    out, ws, x = _buffers()
    res = MG.run_poisoned(lambda: _good(out, ws, x), [out], [ws], [x])
    assert torch.equal(res[0], x * 2 + 1)
    u8 = MG.Guarded.tensor((9,), torch.uint8, CPU)
    MG.run_poisoned(lambda: int(u8.t.fill_(3).sum()) * 0, [u8], poisons=MG.INT_POISONS)


@pytest.mark.parametrize("where,value", [("before", 0x00), ("before", 0xFF), ("after", 0x00), ("after", 0xFF)])
def test_a_byte_outside_the_payload_is_reported_with_its_offset(where, value):
    out, ws, x = _buffers()

    def call():
        _good(out, ws, x)
        if where == "before":
            out.raw[out.off - 1] = value
        else:
            out.raw[out.off + out.nbytes] = value
        return 0

    want = -1 if where == "before" else out.nbytes
    with pytest.raises(AssertionError, match=rf"output 0: guard damaged, first byte at payload offset {want}, last at {want} "):
        MG.run_poisoned(call, [out], [ws], [x])
    assert out.damage() == (want, want)


def test_a_row_of_image_data_behind_the_workspace_is_reported():
    out, ws, x = _buffers()

    def call():
        _good(out, ws, x)
        ws.raw[ws.off + ws.nbytes + 40:ws.off + ws.nbytes + 40 + 96].copy_(x.reshape(-1).view(torch.uint8))
        return 0

    # (131 i + 7) & 0xFF meets a byte of the row by chance now and then: the first and last DIFFERING bytes lie inside the row
    with pytest.raises(AssertionError, match="workspace 0: guard damaged"):
        MG.run_poisoned(call, [out], [ws], [x])
    first, last = ws.damage()
    assert ws.nbytes + 40 <= first <= ws.nbytes + 44 and ws.nbytes + 130 <= last < ws.nbytes + 136


def test_an_unwritten_output_element_is_reported():
    out, ws, x = _buffers()

    def call():
        scratch = ws.view(torch.float32, (4, 6))
        scratch.copy_(x * 2)
        out.t.reshape(-1)[:23].copy_((scratch + 1).reshape(-1)[:23])  # the ragged tail forgets element 23
        return 0

    with pytest.raises(AssertionError, match="output 0 is not finite"):
        MG.run_poisoned(call, [out], [ws], [x])
    # without the NaN poison the comparison across poisons finds it, at its byte
    with pytest.raises(AssertionError, match=r"output 0 differs .*first at byte 92, last at byte 95"):
        MG.run_poisoned(call, [out], [ws], [x], poisons=(MG.POISON_ZERO, MG.POISON_GARBAGE))


def test_a_read_of_unwritten_workspace_is_reported():
    out, ws, x = _buffers()

    def call():
        scratch = ws.view(torch.float32, (4, 6))
        scratch.reshape(-1)[1:].copy_((x * 2).reshape(-1)[1:])  # scratch element 0 is never written ...
        out.t.copy_(scratch * 0 + x)                             # ... and reaches the result through a masked product
        return 0

    with pytest.raises(AssertionError, match="output 0 is not finite"):  # NaN * 0
        MG.run_poisoned(call, [out], [ws], [x])

    def call_byte():
        _good(out, ws, x)
        out.t.view(torch.uint8).reshape(-1)[5] = ws.payload[300]  # a workspace byte nobody wrote
        return 0

    with pytest.raises(AssertionError, match=r"output 0 differs .*\(1 bytes, first at byte 5, last at byte 5\)"):
        MG.run_poisoned(call_byte, [out], [ws], [x], poisons=(MG.POISON_ZERO, MG.POISON_GARBAGE))


def test_a_modified_input_and_a_bad_status_are_reported():
    out, ws, x = _buffers()
    y = x.clone()

    def call():
        _good(out, ws, x)
        y[2, 3] += 1
        return 0

    with pytest.raises(AssertionError, match="input 1 was modified"):
        MG.run_poisoned(call, [out], [ws], [x, y])
    with pytest.raises(AssertionError, match="status -3, expected 0"):
        MG.run_poisoned(lambda: -3, [out], [ws], [x])


def test_an_output_that_doubles_as_an_input_starts_from_its_preset():
    out, ws, x = _buffers()
    out.preset = x.clone()

    def call():
        out.t.mul_(2)
        return 0

    res = MG.run_poisoned(call, [out], [ws], [])
    assert torch.equal(res[0], x * 2) and not out.untouched()
    assert ws.untouched()  # the call never used its workspace


# ---------------------------------------------------------------------------------------------------------------------------------
# every function of include/srx.h that takes a device output pointer has a memory-contract case
# ---------------------------------------------------------------------------------------------------------------------------------
HOST_OUTPUT_FUNCTIONS = {"srx_profile_get"}  # double *total_ms, long *launches: host memory


def device_output_functions():
    """names of the srx.h prototypes with a non-const data pointer parameter other than the workspace (device outputs)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "srx.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    names = []
    for m in re.finditer(r"\bint\s+(srx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        outs = [p for p in params if re.match(r"^(float|double|uint8_t|int)\s*\*\s*\w+$", p)]
        if outs and name not in HOST_OUTPUT_FUNCTIONS:
            names.append(name)
    return names


def test_every_device_output_entry_point_has_a_memory_contract_case():
    import test_gpu_memory_contract as T
    from sr_mi355x import _lib
    parsed = device_output_functions()
    assert len(parsed) >= 40 and "srx_ibp_f32" in parsed and "srx_interleave4_u8" in parsed and "srx_ibp_plan_run" in parsed
    assert set(parsed) <= set(_lib.symbols())
    ids = T.all_case_ids()
    missing = [n for n in parsed if not any(n in i.split("-") for i in ids)]
    assert not missing, f"no memory-contract case in tests/test_gpu_memory_contract.py names {missing}"
    # (functions that write device memory without an output pointer of their own: the plan's create / set_rows)
    for n in ("srx_ibp_plan_create_f32", "srx_ibp_plan_create_f64", "srx_ibp_plan_set_rows_f32", "srx_ibp_plan_set_rows_f64"):
        assert any(n in i.split("-") for i in ids), n


def _route(c, prec):
    """srx_ibp_path_for: the path the library routes this configuration to in `prec` (host arithmetic, no device)"""
    import numpy as np
    import test_gpu_memory_contract as T
    from sr_mi355x import _lib
    (h, w), f = c["hw"], c["f"]
    sh = np.ascontiguousarray(np.asarray(c["shifts"], dtype=np.float64))
    k = np.ascontiguousarray(np.asarray(T._PSF[c["psf"]], dtype=np.float64))
    return _lib.load().srx_ibp_path_for({"f32": 4, "f64": 8}[prec], len(sh), h, w, h * f, w * f, f, sh.ctypes.data_as(_lib._HD),
                                        k.ctypes.data_as(_lib._HD), k.shape[0], k.shape[1], c["flags"]).decode()


def test_every_ibp_case_routes_to_the_path_it_names():
    """... asked of the library's own router, so a configuration that names the wrong path fails here, without a GPU"""
    import test_gpu_memory_contract as T
    wrong = [(T._ibp_id(c), _route(c, c["prec"])) for c in T.IBP_CASES if _route(c, c["prec"]) != c["path"]]
    assert not wrong, wrong


def test_every_path_is_declared_in_every_precision_it_admits():
    """The ten names of srx_last_path() (srx.h) all have a case, and so has every (path, precision) pair the router admits: each case's
    configuration is routed in the OTHER precision too, and where it lands is a pair that needs a case of its own -- if the route table
    gains a precision for a path, this fails until the GPU file declares it."""
    import test_gpu_memory_contract as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "include", "srx.h")).read()
    doc = doc[doc.index("Name of the code path"):doc.index("const char *srx_last_path")]
    names = set(re.findall(r'"(\w+)"', doc))
    assert len(names) == 10
    declared = {(c["path"], c["prec"]) for c in T.IBP_CASES}
    assert {pth for pth, _ in declared} == names
    admitted = {(_route(c, pr), pr) for c in T.IBP_CASES for pr in ("f32", "f64")}
    assert admitted <= declared, f"admitted by the router, without a memory-contract case: {sorted(admitted - declared)}"
    # the precisions known today (csrc/srx_route.hpp, route_ibp): the derivation above must at least see these
    assert {("ctile", "f32"), ("ctile", "f64"), ("mosaic", "f32"), ("mosaic", "f64"), ("fused", "f32"), ("fused", "f64"), ("composed", "f32"),
            ("composed", "f64"), ("patch", "f32"), ("stile", "f64"), ("ztile", "f32"), ("dtile", "f32"), ("atile", "f32"), ("btile", "f32")} <= admitted
