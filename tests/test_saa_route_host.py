"""The route of a shift_and_add call, checked without a GPU: srx_saa_path_for answers from the record the call itself reads (route_saa),
and a refused call returns before anything is queued (the device pointers below are placeholders nobody follows).

The expected names follow fused::saa_eligible (N <= 32, f >= 1, frames of at least 2 x 2, |f s| <= 4 HR px) and mosaic::saa_eligible
(that, f in 2..4, frames of at least 8 x 8, one sub-pixel fraction per axis)."""
import numpy as np
import pytest

from sr_mi355x import _lib, synth
from test_items_host import EB, FAKE, LARGE, _lib_max_frames, hd, lib

H, W, N = 40, 56, 4


def path_for(prec, table, f, flags=0, h=H, w=W):
    sh, shp = hd(table)
    return lib().srx_saa_path_for(EB[prec], len(sh), h, w, f, shp, flags).decode()


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_path_names(prec):
    assert path_for(prec, synth.NOMINAL_4, 2) == "mosaic"
    assert path_for(prec, synth.NOMINAL_4, 4) == "mosaic"
    assert path_for(prec, synth.NOMINAL_4, 2, _lib.FLAG_PER_FRAME) == "fused"
    assert path_for(prec, synth.NOMINAL_4, 2, _lib.FLAG_COMPOSED) == "composed"
    assert path_for(prec, synth.NOMINAL_4, 1) == "fused"  # the mosaic form takes factors 2..4
    assert path_for(prec, synth.NOMINAL_4, 2, h=6) == "fused"  # ... and needs 8 rows
    assert path_for(prec, synth.MEASURED_4, 2) == "fused"
    assert path_for(prec, LARGE, 2) == "composed"
    assert path_for(prec, LARGE, 2, _lib.FLAG_FUSED) == "none"
    assert path_for(prec, np.zeros((_lib_max_frames() + 1, 2)), 2) == "none"
    assert path_for(prec, synth.NOMINAL_4, 2, h=0) == "none"


@pytest.mark.parametrize("prec", ["f32", "f64"])
def test_status_order(prec):
    """SRX_FLAG_FUSED on a table that cannot fuse, and a workspace one byte short: the shared-table and uint8 entries answer the workspace
    first, the per-item entry the flag; with the workspace they ask for, all answer the flag."""
    L, B, f = lib(), 2, 2
    one, onep = hd(LARGE)
    per, perp = hd(np.stack([LARGE] * B))
    entries = [(f"srx_saa_{prec}", L.srx_saa_workspace_bytes, onep, _lib.E_WORKSPACE),
               (f"srx_saa_u8lr_{prec}", L.srx_saa_u8lr_workspace_bytes, onep, _lib.E_WORKSPACE),
               (f"srx_saa_items_{prec}", L.srx_saa_items_workspace_bytes, perp, _lib.E_UNSUPPORTED)]
    for name, query, shp, short in entries:
        need = query(EB[prec], B, N, H, W, f)
        call = lambda wsb: getattr(L, name)(FAKE, B, N, H, W, shp, f, FAKE, FAKE, wsb, None, _lib.FLAG_FUSED)  # noqa: E731
        assert call(need - 1) == short, name
        assert call(need) == _lib.E_UNSUPPORTED, name
