"""The stream and graph contract of include/srx.h, entry point by entry point: every function that takes an srx_stream_t is called on a
side stream inside a HIP stream capture and must queue kernels and device-to-device copies on that stream and nothing else -- nothing
runs eagerly, no memset / host / mem-alloc node, the documented kernel-node counts, the same node list whatever the samples hold -- and
the captured call, launched once on samples, host tables and device-side parameters it has not seen, must give the bits of a plain call
(tests/streamcheck.py has the steps, tests/stream_contract_cases.py the table; tests/test_stream_contract_host.py compares the table
with the header).  tests/test_gpu_memory_contract.py is the other half of the header's promise.

Launches of an instantiated graph run in a fresh child process with DEBUG_CLR_GRAPH_PACKET_CAPTURE=0, exactly as tests/test_gpu_graph.py
does and for the reason given there and in profiles/README.md; no other runtime variable is set.  One worker runs at a time."""
import json
import os
import subprocess
import sys

import pytest

import stream_contract_cases as C

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

# family: wall time of its worker, measured once on an MI355X (seconds; process start and library load dominate and vary).  The limit of a
# worker is the larger of 60 s and 5 times that.
MEASURED = {"prims": 2.7, "saa": 2.4, "ibp": 2.7, "plan": 2.3, "metrics": 2.4, "register_psf": 2.3, "png_crc": 2.4, "patches": 2.5,
            "selftest": 2.2}


def limit(family):
    return max(60.0, 5.0 * MEASURED[family])


def worker(family):
    env = dict(os.environ, DEBUG_CLR_GRAPH_PACKET_CAPTURE="0")
    r = subprocess.run([sys.executable, os.path.join(HERE, "stream_contract_worker.py"), family], env=env, capture_output=True, text=True,
                       timeout=limit(family))
    lines = r.stdout.strip().splitlines()
    assert lines, f"the worker printed nothing (exit status {r.returncode}): {r.stderr[-2000:]}"
    res = json.loads(lines[-1])
    for cid, v in res.items():
        print(f"{cid}: {v['nodes']}" + (f"  -- {v['detail']}" if v["detail"] else ""))
    return r, res


@pytest.mark.parametrize("family", C.FAMILIES)
def test_family(family):
    r, res = worker(family)
    bad = {k: v["detail"] for k, v in res.items() if not v["ok"]}
    assert not bad, bad
    assert list(res) == C.family_ids(family), f"the worker stopped early or ran other cases (exit status {r.returncode}): {r.stderr[-2000:]}"
    assert r.returncode == 0, r.stderr[-2000:]


def test_the_checker_reports_each_planted_violation():
    """stand-in callees (torch ops and plain HIP calls, none of them faults): work sent to another stream, a hipMemsetAsync on the capture
    stream and a parameter baked in at capture are each reported with their reason; a sound callee -- a kernel and a device-to-device
    copy -- passes"""
    r, res = worker("selftest")
    assert list(res) == list(C.SELFTEST) and r.returncode == 0, r.stderr[-2000:]
    for cid, (_, reason) in C.SELFTEST.items():
        if reason is None:
            assert res[cid]["ok"], res[cid]
        else:
            assert not res[cid]["ok"] and reason in res[cid]["detail"], (cid, res[cid])
    assert res["standin-sound"]["nodes"]["kernel"] == 1 and res["standin-sound"]["nodes"]["memcpy"] == 1
    assert res["standin-other_stream"]["nodes"]["kernel"] == 0
    assert "memset" in res["standin-memset"]["nodes"]["all"]
