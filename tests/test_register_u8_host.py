"""srx_register_u8_* without a GPU: the symbols and their signature, estimate_shifts' argument errors on uint8 input (raised before any
device work, the float input's errors word for word), and what session.register_shifts hands to estimate_shifts."""
import numpy as np
import pytest
import torch

from sr_mi355x import _lib, api, session
from sr_mi355x import register as G


def test_symbols_and_signature():
    assert {"srx_register_u8_f32", "srx_register_u8_f64"} <= set(_lib.symbols())
    assert _lib._TYPED["srx_register_u8_{T}"] == _lib._TYPED["srx_register_{T}"]
    lib = _lib.load()
    for t in ("f32", "f64"):
        fn, ff = getattr(lib, f"srx_register_u8_{t}"), getattr(lib, f"srx_register_{t}")
        assert fn.argtypes == ff.argtypes and fn.restype == ff.restype


BAD = [
    ((4, 40, 40), dict(ref=4)),
    ((4, 40, 40), dict(ref=-1)),
    ((4, 40, 40), dict(search=5)),
    ((4, 40, 40), dict(search=-1)),
    ((4, 40, 40), dict(border=-1)),
    ((4, 40, 40), dict(search=2, border=9)),   # crop 40 - 2 (9 + 2 + 2) = 14
    ((4, 39, 64), dict(search=2, border=8)),   # crop 15 x 40
    ((1, 40, 40), dict()),                     # N < 2
    ((4, 40, 40), dict(init=np.zeros((3, 2)))),
    ((2, 4, 40, 40), dict(init=np.zeros((2, 4, 2)))),
    ((4, 40, 40), dict(n_iter=-1)),
    ((4, 40, 40), dict(tol=float("nan"))),
]


@pytest.mark.parametrize("shape,kw", BAD, ids=[f"{'x'.join(map(str, s))}-{'-'.join(f'{k}' for k in kw) or 'N'}" for s, kw in BAD])
def test_argument_errors_are_the_float_input_s(shape, kw):
    msgs = []
    for frames in (np.zeros(shape, np.uint8), np.zeros(shape, np.float64), torch.zeros(shape, dtype=torch.uint8), [np.zeros(shape[1:], np.uint8)] * shape[0]):
        with pytest.raises(ValueError) as e:
            G.estimate_shifts(frames, **kw)
        msgs.append(str(e.value))
    assert len(set(msgs)) == 1, msgs


def test_uint8_detection():
    u, f = np.zeros((2, 3, 3), np.uint8), np.zeros((2, 3, 3))
    assert api._is_u8(u) and api._is_u8(torch.from_numpy(u)) and api._is_u8(list(u)) and api._is_u8([torch.from_numpy(a) for a in u])
    assert not api._is_u8(f) and not api._is_u8(torch.from_numpy(f)) and not api._is_u8(list(f)) and not api._is_u8([u[0], f[1]])
    assert not api._is_u8(u.astype(np.int8)) and not api._is_u8(u.tolist())


def test_register_shifts_hands_bytes_on_as_bytes(monkeypatch):
    seen = []

    def fake(frames, init=None, full=False, **kw):
        assert full and not kw
        seen.append((frames.dtype, tuple(frames.shape)))
        B, N = frames.shape[:2]
        est = np.broadcast_to(np.asarray(init, np.float64), (B, N, 2)) + 0.25
        status = np.zeros((B, N), np.int32)
        status[:, 1] = 3
        return est, np.full((B, N), 0.5), status

    monkeypatch.setattr(G, "estimate_shifts", fake)
    table = [(0.0, 0.0), (0.5, -0.5), (-0.5, 0.5)]
    for dt in (torch.uint8, torch.float64, torch.float32):
        sets = [[torch.zeros((20, 24), dtype=dt) for _ in range(3)] for _ in range(2)]
        out = session.register_shifts(sets, table)
        assert seen[-1] == (dt, (2, 3, 20, 24))
        assert len(out) == 2
        used, rep = out[0]
        assert used == [(0.25, 0.25), (0.5, -0.5), (-0.25, 0.75)]  # a nonzero status keeps the table shift
        assert rep["status"] == [0, 3, 0] and rep["nominal"] == [list(s) for s in table]
