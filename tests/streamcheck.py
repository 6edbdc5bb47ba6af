"""The stream and graph contract of include/srx.h ("Conventions", "Streams and graphs"), checked for one C-ABI call: the checker behind
tests/stream_contract_worker.py, the counterpart of tests/memguard.py.  A plain helper module: no fixtures, nothing registered.

The header promises that a call queues kernels and device-to-device copies on `stream` and nothing else: no synchronisation, no allocation,
no memset node, no host copy, the host arrays read before the call returns, the implementation and the launch count decided without the
samples.  A test that passes the default stream and synchronises before it looks cannot see a violation of any of this.  So, per case:

  capture   the call is made on a side stream inside hipStreamBeginCapture(global) -- nothing else is captured -- after one plain call on
            that stream (lazy module loading stays out of the capture), into outputs and a workspace filled with a poison;
  eager     after the capture and a device synchronise every byte of the outputs and of the workspace still holds the poison and the
            inputs are intact: work that went to another stream ran, and shows, whatever the runtime does with such launches;
  census    hipGraphGetNodes / hipGraphNodeGetType: kernel nodes and device-to-device memcpy nodes only (copies only where the case allows
            them), the kernel-node count srx.h documents, and the same node list from a second capture on other samples;
  launch    the graph is instantiated and launched ONCE on data the capture has not seen -- new samples in the device inputs, every host
            array the call took overwritten in place with a permuted copy, the outputs and the workspace re-poisoned with another byte --
            and the written part of every output must equal, bit for bit, a plain call on the default stream with buffers and (original)
            host arrays of its own; once more with a third, not integer-valued sample set.

A case is described by a builder that returns an Inst (the call as a closure over preallocated buffers); the checker builds two of them,
one to capture and one for the plain calls.  The graph API is bound with ctypes to the libamdhip64 the process has mapped already (its
path is read from /proc/self/maps after `import torch`): a second copy of the runtime would own none of the streams and pointers in use
(sr_mi355x._lib.load()).  Every HIP status is checked; the first one that is not hipSuccess raises HipFailure, after which the caller
starts no further GPU work (tests/stream_contract_worker.py reports what it has and exits)."""
import ctypes
import os
import re
import tempfile

import numpy as np
import torch

import memguard as MG

KERNEL, MEMCPY, MEMSET, HOST, MEMALLOC = 0, 1, 2, 3, 10
NODE_NAMES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "child graph", 5: "empty", 6: "event wait", 7: "event record",
              8: "semaphore signal", 9: "semaphore wait", 10: "mem-alloc", 11: "mem-free", 12: "memcpy from symbol", 13: "memcpy to symbol",
              14: "batch mem-op"}
KIND_NAMES = {0: "HtoH", 1: "HtoD", 2: "DtoH", 3: "DtoD", 1024: "DtoD"}  # hipMemcpyKind (1024: device-to-device without compute units)
CAPTURE_GLOBAL = 0
POISON_CAPTURE, POISON_LAUNCH = MG.POISON_NAN, (MG.POISON_GARBAGE, MG.POISON_ZERO)


class HipFailure(RuntimeError):
    """a HIP call of the checker itself did not return hipSuccess: nothing more is started on the device"""


class _Pos(ctypes.Structure):
    _fields_ = [("x", ctypes.c_size_t), ("y", ctypes.c_size_t), ("z", ctypes.c_size_t)]


class _PitchedPtr(ctypes.Structure):
    _fields_ = [("ptr", ctypes.c_void_p), ("pitch", ctypes.c_size_t), ("xsize", ctypes.c_size_t), ("ysize", ctypes.c_size_t)]


class Memcpy3DParms(ctypes.Structure):  # hip/driver_types.h
    _fields_ = [("srcArray", ctypes.c_void_p), ("srcPos", _Pos), ("srcPtr", _PitchedPtr), ("dstArray", ctypes.c_void_p), ("dstPos", _Pos),
                ("dstPtr", _PitchedPtr), ("extent", _Pos), ("kind", ctypes.c_int)]


_hip = None


def mapped_runtime_path():
    """the libamdhip64 this process has mapped (torch's own copy once torch is imported)"""
    with open("/proc/self/maps") as f:
        for line in f:
            m = re.search(r"(/\S*libamdhip64\.so[^\s]*)", line)
            if m:
                return m.group(1)
    raise RuntimeError("no libamdhip64 is mapped: import torch (ROCm) first")


def hip():
    global _hip
    if _hip is None:
        lib = ctypes.CDLL(mapped_runtime_path())  # the path of a mapped object: dlopen returns the copy already loaded
        P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
        for name, args in {"hipStreamBeginCapture": [P, I], "hipStreamEndCapture": [P, ctypes.POINTER(P)],
                           "hipGraphGetNodes": [P, ctypes.POINTER(P), ctypes.POINTER(Z)], "hipGraphNodeGetType": [P, ctypes.POINTER(I)],
                           "hipGraphMemcpyNodeGetParams": [P, ctypes.POINTER(Memcpy3DParms)],
                           "hipGraphInstantiate": [ctypes.POINTER(P), P, P, P, Z], "hipGraphLaunch": [P, P], "hipGraphExecDestroy": [P],
                           "hipGraphDestroy": [P], "hipStreamSynchronize": [P], "hipDeviceSynchronize": [], "hipMemsetAsync": [P, I, Z, P],
                           "hipMemcpyAsync": [P, P, Z, I, P], "hipGraphDebugDotPrint": [P, ctypes.c_char_p, ctypes.c_uint]}.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = I, args
        lib.hipGetErrorString.restype, lib.hipGetErrorString.argtypes = ctypes.c_char_p, [I]
        _hip = lib
    return _hip


def ok(status, what):
    if status != 0:
        raise HipFailure(f"{what}: HIP status {status} ({hip().hipGetErrorString(status).decode()})")


def sync():
    ok(hip().hipDeviceSynchronize(), "hipDeviceSynchronize")


def permuted(a):
    """a different valid table of the same values: the flat array reversed and rotated by one (or, where that gives the array back -- a
    table symmetric about its middle -- reversed only, or rotated only)"""
    flat = np.asarray(a).ravel()
    for b in (np.roll(flat[::-1], 1), flat[::-1], np.roll(flat, 1)):
        if not np.array_equal(flat, b):
            return b.reshape(np.shape(a)).copy()
    raise AssertionError("every permuted copy of a host array equals the array: give the case a table with distinct entries")


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


class Inst:
    """One call with everything it touches preallocated.
      call(stream_ptr) -> status   the C-ABI call (stream_ptr: an int, or None for the default stream)
      ins        device tensors the call reads; samples(k) -> the tensors of sample set k = 0, 1, 2 to copy into them (device-side
                 parameters -- srx_crc32's lengths, srx_ssim's affine -- are inputs like the others)
      outs       device tensors the call writes; written(outs) -> the tensors to compare (default: the outputs whole)
      ws         the workspace tensor (uint8) or None
      host       the host float64 arrays the call took pointers of (overwritten in place before a launch)
      path       the name srx_last_path() must report after the call, or None
      cleanup    called once when the case is over (plans are destroyed here, after the launches)"""

    def __init__(self, call, ins, samples, outs, ws=None, host=(), path=None, written=None, cleanup=None):
        self.call, self.ins, self.samples, self.outs, self.ws = call, list(ins), samples, list(outs), ws
        self.host, self.path, self.written, self.cleanup = list(host), path, written or (lambda outs: list(outs)), cleanup
        self.poison, self.get_path = None, None   # get_path: where the path is not srx_last_path()'s (a plan's)

    def load(self, k):
        for x, s in zip(self.ins, self.samples(k)):
            assert x.shape == s.shape and x.dtype == s.dtype
            x.copy_(s)

    def fill(self, poison):
        self.poison = poison
        for t in self.outs + ([self.ws] if self.ws is not None else []):
            assert t.is_contiguous()
            _bytes(t).fill_(poison)

    def untouched(self):
        """names of the buffers that no longer hold their poison, byte for byte"""
        bad = [f"output {i}" for i, t in enumerate(self.outs) if not bool((_bytes(t) == self.poison).all())]
        if self.ws is not None and not bool((self.ws == self.poison).all()):
            bad.append("workspace")
        return bad

    def swap_host(self):
        for a in self.host:
            a[...] = permuted(a)


def capture(inst, side, last_path=None):
    """the call alone inside a global-mode capture on `side` -> (graph handle, status of the call, srx_last_path() or None)"""
    h = hip()
    sp = ctypes.c_void_p(side.cuda_stream)
    graph = ctypes.c_void_p()
    ok(h.hipStreamBeginCapture(sp, CAPTURE_GLOBAL), "hipStreamBeginCapture")
    try:
        with torch.cuda.stream(side):
            status = inst.call(side.cuda_stream)
        get = inst.get_path or last_path
        path = get() if (inst.path is not None and get is not None) else None
    finally:
        rc = h.hipStreamEndCapture(sp, ctypes.byref(graph))
    ok(rc, "hipStreamEndCapture")
    return graph, status, path


def dot_directions(graph):
    """the directions ("DtoD", "HtoD", ...) hipGraphDebugDotPrint writes into the labels of the graph's memcpy nodes, in file order"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "graph.dot")
        if hip().hipGraphDebugDotPrint(graph, path.encode(), 0) != 0 or not os.path.exists(path):
            return []
        with open(path) as f:
            return re.findall(r"\b(DtoD|HtoD|DtoH|HtoH)\b", f.read())


def census(graph):
    """-> (node types in the order hipGraphGetNodes gives them, the direction of every memcpy node).  A direction is "DtoD", "HtoD", "DtoH",
    "HtoH" or None.  hipGraphMemcpyNodeGetParams answers for nodes that were added with hipMemcpy3DParms; for a node captured from
    hipMemcpyAsync (the only copies the library makes) ROCm 7.2 returns a structure it never filled -- the `kind` read back from one and
    the same device-to-device copy was 0 in one capture and -1261024224 in the next -- so such a node's direction is taken from the label
    hipGraphDebugDotPrint gives it, and is None ("the runtime does not say") where that has none either.  The label is a weak witness: a
    copy from page-locked host memory is labelled "DtoD" as well.  What holds a call to "no host copy" is therefore the launch on
    overwritten host arrays (the "host_copy" stand-in of the self-test: its graph passes this census and fails that comparison)."""
    h = hip()
    n = ctypes.c_size_t(0)
    ok(h.hipGraphGetNodes(graph, None, ctypes.byref(n)), "hipGraphGetNodes (count)")
    if n.value == 0:
        return [], []
    nodes = (ctypes.c_void_p * n.value)()
    ok(h.hipGraphGetNodes(graph, nodes, ctypes.byref(n)), "hipGraphGetNodes")
    types = []
    for i in range(n.value):
        t = ctypes.c_int(-1)
        ok(h.hipGraphNodeGetType(ctypes.c_void_p(nodes[i]), ctypes.byref(t)), "hipGraphNodeGetType")
        types.append(t.value)
    ncopy = types.count(MEMCPY)
    kinds = dot_directions(graph) if ncopy else []
    if len(kinds) != ncopy:   # no label per copy node: ask the node itself, and believe it only where the structure was filled
        kinds = []
        for i in range(n.value):
            if types[i] == MEMCPY:
                prm = Memcpy3DParms()
                ok(h.hipGraphMemcpyNodeGetParams(ctypes.c_void_p(nodes[i]), ctypes.byref(prm)), "hipGraphMemcpyNodeGetParams")
                filled = prm.kind in KIND_NAMES and prm.extent.x > 0 and bool(prm.srcPtr.ptr) and bool(prm.dstPtr.ptr)
                kinds.append(KIND_NAMES[prm.kind] if filled else None)
    return types, kinds


def describe(types):
    return ", ".join(f"{types.count(t)} {NODE_NAMES.get(t, t)}" for t in sorted(set(types))) or "no node"


def judge(types, kinds, kernels=None, copies=0):
    """the census rules -> list of complaints.  kernels: None (not numbered by srx.h), an int, or ("max", n); copies: how many
    device-to-device memcpy nodes the case allows (None: any number)"""
    bad = []
    for t in sorted(set(types) - {KERNEL, MEMCPY}):
        bad.append(f"{types.count(t)} {NODE_NAMES.get(t, t)} node(s) in the captured call")
    for k in kinds:
        if k is not None and k != "DtoD":
            bad.append(f"a {k} memcpy node, not device-to-device")
    nk, nc = types.count(KERNEL), types.count(MEMCPY)
    if copies is not None and nc > copies:
        bad.append(f"{nc} memcpy node(s) where {copies} are allowed")
    if isinstance(kernels, int) and nk != kernels:
        bad.append(f"{nk} kernel nodes, srx.h documents {kernels}")
    if isinstance(kernels, tuple) and nk > kernels[1]:
        bad.append(f"{nk} kernel nodes, srx.h documents at most {kernels[1]}")
    return bad


def count_nodes(make, side, **kw):
    """node types of one capture of make(**kw) (after its own warm-up call); the graph is destroyed, never launched"""
    inst = make(**kw)
    try:
        inst.load(0)
        with torch.cuda.stream(side):
            st = inst.call(side.cuda_stream)
        sync()
        if st != 0:
            return None, f"status {st} with {kw}"
        graph, st, _ = capture(inst, side)
        types, _ = census(graph)
        ok(hip().hipGraphDestroy(graph), "hipGraphDestroy")
        sync()
        return (types, None) if st == 0 else (None, f"status {st} inside the capture with {kw}")
    finally:
        if inst.cleanup:
            inst.cleanup()


def check(make, kernels=None, copies=0, exact_copies=None, diffs=(), last_path=None, profile_off=None):
    """Run one case.  make(**kw) -> Inst.  diffs: (kw_a, kw_b, expected): the nodes of make(**kw_a) minus those of make(**kw_b); expected is
    the kernel-node difference, a pair (kernel nodes, memcpy nodes), or None (reported only).
    -> {"ok", "nodes": {"kernel", "memcpy", "all", "diffs"}, "detail"}, with "stop": True where the call itself returned an error (the caller
    goes no further then).  HipFailure passes through."""
    if profile_off is not None:
        profile_off()
    h = hip()
    detail, nodes = [], {}
    side = torch.cuda.Stream()
    cap, ref = make(), make()
    graph = gexec = None
    try:
        # 1. warm-up on the side stream
        cap.load(0)
        sync()
        with torch.cuda.stream(side):
            st = cap.call(side.cuda_stream)
        sync()
        if st != 0:
            return {"ok": False, "stop": True, "nodes": nodes, "detail": f"warm-up call: status {st}"}
        # 2. capture into poisoned buffers
        cap.fill(POISON_CAPTURE)
        before = [x.clone() for x in cap.ins]
        sync()
        graph, st, path = capture(cap, side, last_path)
        sync()
        if st != 0:
            return {"ok": False, "stop": True, "nodes": nodes, "detail": f"status {st} inside the capture"}
        if cap.path is not None and path != cap.path:
            detail.append(f"path {path}, expected {cap.path}")
        # 3. nothing ran eagerly
        touched = cap.untouched()
        if touched:
            detail.append("written during the capture: " + ", ".join(touched))
        if not all(torch.equal(a, b) for a, b in zip(cap.ins, before)):
            detail.append("an input was modified during the capture")
        # 4. the node census, and the same list from a capture on other samples
        types, kinds = census(graph)
        nodes = {"kernel": types.count(KERNEL), "memcpy": types.count(MEMCPY), "all": describe(types), "copies": kinds}
        detail += judge(types, kinds, kernels, copies)
        if exact_copies is not None and types.count(MEMCPY) != exact_copies:
            detail.append(f"{types.count(MEMCPY)} memcpy node(s), expected {exact_copies}")
        cap.load(1)
        sync()
        g2, st, _ = capture(cap, side)
        types2, _ = census(g2)
        ok(h.hipGraphDestroy(g2), "hipGraphDestroy")
        sync()
        if st != 0:
            return {"ok": False, "stop": True, "nodes": nodes, "detail": f"status {st} inside the second capture"}
        if types2 != types:
            detail.append(f"the node list depends on the samples: {describe(types)} / {describe(types2)}")
        if cap.untouched():
            detail.append("written during the second capture: " + ", ".join(cap.untouched()))
        nodes["diffs"] = []
        for kw_a, kw_b, want in diffs:
            ta, ea = count_nodes(make, side, **kw_a)
            tb, eb = count_nodes(make, side, **kw_b)
            if ea or eb:
                detail.append(ea or eb)
                continue
            d = (ta.count(KERNEL) - tb.count(KERNEL), ta.count(MEMCPY) - tb.count(MEMCPY))
            nodes["diffs"].append(list(d))
            if want is not None and d != (want if isinstance(want, tuple) else (want, d[1])):
                detail.append(f"{d[0]} kernel and {d[1]} memcpy nodes between {kw_a} and {kw_b}, srx.h documents {want}")
            if set(ta + tb) - {KERNEL, MEMCPY}:
                detail.append(f"{kw_a} / {kw_b}: {describe(ta)} / {describe(tb)}")
        # 5., 6. one launch each on data the capture has not seen
        gexec = ctypes.c_void_p()
        ok(h.hipGraphInstantiate(ctypes.byref(gexec), graph, None, None, 0), "hipGraphInstantiate")
        cap.swap_host()
        for k, poison in zip((1, 2), POISON_LAUNCH):
            cap.load(k)
            cap.fill(poison)
            sync()
            ok(h.hipGraphLaunch(gexec, ctypes.c_void_p(side.cuda_stream)), "hipGraphLaunch")
            ok(h.hipStreamSynchronize(ctypes.c_void_p(side.cuda_stream)), "hipStreamSynchronize after hipGraphLaunch")
            sync()
            ref.load(k)
            ref.fill(POISON_CAPTURE)
            sync()
            st = ref.call(None)
            sync()
            if st != 0:
                detail.append(f"sample set {k}: the plain call returned status {st}")
                continue
            got, want = cap.written(cap.outs), ref.written(ref.outs)
            for i, (a, b) in enumerate(zip(got, want)):
                if a.shape != b.shape or a.dtype != b.dtype:
                    detail.append(f"sample set {k}: output {i} has another extent than the plain call's ({tuple(a.shape)} / {tuple(b.shape)})")
                    continue
                ne = _bytes(a) != _bytes(b)
                if bool(ne.any()):
                    idx = ne.nonzero().flatten()
                    detail.append(f"sample set {k}: output {i} differs from the plain call in {int(idx.numel())} bytes, first at byte {int(idx[0])}")
            if not all(torch.equal(x, s) for x, s in zip(cap.ins, cap.samples(k))):
                detail.append(f"sample set {k}: an input was modified by the launch")
    finally:
        if gexec is not None and gexec.value:
            h.hipGraphExecDestroy(gexec)
        if graph is not None and graph.value:
            h.hipGraphDestroy(graph)
        for inst in (cap, ref):
            if inst.cleanup:
                inst.cleanup()
    return {"ok": not detail, "nodes": nodes, "detail": "; ".join(detail)}
