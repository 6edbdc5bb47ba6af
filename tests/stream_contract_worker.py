"""Worker of tests/test_gpu_stream_contract.py (a process of its own: the HIP runtime reads DEBUG_CLR_GRAPH_PACKET_CAPTURE once, when it
loads, and launches of an instantiated graph run with it off, as in tests/graph_replay_worker.py).

    python stream_contract_worker.py FAMILY [case id ...]

runs the cases of one family of tests/stream_contract_cases.py ("selftest": the stand-in callees that prove the checker) through
tests/streamcheck.py and prints one JSON line {case id: {"ok": bool, "nodes": {...}, "detail": str}}.  The first HIP call of the checker
that fails, a captured call that returns an error and any exception end the run there: the line then holds the cases finished so far
(plus the one that stopped it, not ok), the exit status is 3 and nothing more is started on the device."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "enph459-super-resolution_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402,F401  (first: the graph API is bound to the runtime torch has loaded)
import stream_contract_cases as C  # noqa: E402
import streamcheck as SC  # noqa: E402


def run(family, only=()):
    lib = C.T.lib()
    if family == "selftest":
        todo = [(cid, dict(make=mk, copies=None)) for cid, (mk, _) in C.SELFTEST.items()]
    else:
        todo = [(c.id, dict(make=c.make, kernels=c.kernels, copies=c.copies, exact_copies=c.exact_copies, diffs=c.diffs))
                for c in C.CASES.values() if c.family == family]
    res, stopped = {}, False
    for cid, kw in todo:
        if only and cid not in only:
            continue
        try:
            res[cid] = SC.check(last_path=C.last_path, profile_off=lambda: lib.srx_profile_enable(0), **kw)
            stopped = bool(res[cid].pop("stop", False))
        except Exception as e:  # noqa: BLE001  (HipFailure, a torch error after a device fault, a builder's assertion: stop either way)
            res[cid] = {"ok": False, "nodes": {}, "detail": f"{type(e).__name__}: {e}"[:600]}
            stopped = True
        if stopped:
            break
    return res, stopped


if __name__ == "__main__":
    results, stop = run(sys.argv[1], sys.argv[2:])
    print(json.dumps(results), flush=True)
    sys.exit(3 if stop else 0)
