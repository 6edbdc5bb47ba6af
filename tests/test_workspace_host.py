"""Every workspace query of include/srx.h against tests/golden/workspace_bytes.txt, line by line, without a GPU.

The golden file is the reduced sweep of tools/ws_sweep.py (every *_workspace_bytes and *_workspace_bytes_for query, srx_ibp_path_for and
srx_saa_path_for; every case of IBP_CASES, so every value of srx_last_path()), printed by the library of the commit BEFORE the workspace
layouts became one function per driver (carve on the call's arena, the same carve measured for the query).  A change that means to alter a
returned size regenerates it with `python3 tools/ws_sweep.py --reduced` on the parent's build and says so; the memory-contract GPU tests then
hold every call to the new figure.
"""
import os
import sys

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ws_sweep  # noqa: E402
from sr_mi355x import _lib  # noqa: E402


def test_every_workspace_query_returns_the_golden_size():
    want = open(os.path.join(GOLDEN, "workspace_bytes.txt")).read().splitlines()
    got = list(ws_sweep.sweep(_lib.load(), ws_sweep.REDUCED))  # (asserts on its own that all ten paths were met and no line skipped)
    assert 300 <= len(want) and len(got) == len(want)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} lines differ; the first: got {wrong[0][0]!r}, golden {wrong[0][1]!r}"


def test_the_golden_sweep_names_every_query_and_every_path():
    want = open(os.path.join(GOLDEN, "workspace_bytes.txt")).read().splitlines()
    names = {ln.split(" ", 1)[0] for ln in want}
    queries = {n for n in _lib.symbols() if n.endswith("_workspace_bytes") or n.endswith("_workspace_bytes_for")}
    assert len(queries) == 17 and queries | {"srx_ibp_path_for", "srx_saa_path_for"} == names
    paths = {ln.rsplit(" -> ", 1)[1] for ln in want if ln.startswith("srx_ibp_path_for ")}
    assert paths == ws_sweep.PATHS
