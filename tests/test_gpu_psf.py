"""srx_psf_estimate_{u8,f32,f64} on the device (csrc/srx_psf.hpp) against the reference's own kernel (tests/golden/pinholes.npz: psf_m is
what load_measured_psf, mono_cal_target/run_sr.py:114-152, made of those windows), np.argmax, the host form
session.psf_from_pinhole_images, and the library's memory contract.

Shapes are the smallest at which the arg-max kernel can still go wrong: a workgroup takes CHUNK_BYTES = 32 KiB of one frame, peels the samples
in front of the first 16-byte boundary and behind the last whole vector, so the frames span three chunks with a ragged last one, H W is
odd (every frame of a stack starts at another alignment) and every single-maximum case is run at four consecutive frame slots.
"""
import ctypes

import numpy as np
import pytest
import torch

import memguard as MG
import test_gpu_memory_contract as T
from conftest import load_golden
from sr_mi355x import _lib, api, psf_device, session

pytestmark = pytest.mark.gpu

CUDA = "cuda"
NP_DT = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}
TORCH_DT = {"u8": torch.uint8, "f32": torch.float32, "f64": torch.float64}
EB = {"u8": 1, "f32": 4, "f64": 8}
KINDS = ("u8", "f32", "f64")
EMBED = (131, 203)  # odd H W: every other frame of a uint8 stack starts at an odd byte


def entry(kind):
    return getattr(_lib.load(), f"srx_psf_estimate_{kind}")


def need_bytes(kind, N, H, W, halfwidth):
    n = _lib.load().srx_psf_estimate_workspace_bytes(EB[kind], N, H, W, halfwidth)
    assert n > 0
    return n


def run(x, kind, halfwidth=3):
    """one call on a device stack [N, H, W] -> (psf float64 [side, side], info int32 [N, 3]) on the host"""
    N, H, W = x.shape
    side = 2 * halfwidth + 1
    psf = torch.full((side, side), float("nan"), dtype=torch.float64, device=CUDA)
    info = torch.full((N, 3), -7, dtype=torch.int32, device=CUDA)
    n = need_bytes(kind, N, H, W, halfwidth)
    ws = torch.empty(n, dtype=torch.uint8, device=CUDA)
    st = entry(kind)(T.p(x), N, H, W, halfwidth, T.p(psf), T.p(info), T.p(ws), ctypes.c_size_t(n), api._stream())
    assert st == _lib.OK, st
    return psf.cpu().numpy(), info.cpu().numpy()


def dev(a, kind):
    return torch.from_numpy(np.ascontiguousarray(a).astype(NP_DT[kind])).to(CUDA)


def argmax_rc(a):
    return np.array([np.unravel_index(np.argmax(f), f.shape) for f in a], dtype=np.int64)


@pytest.fixture(scope="module")
def golden():
    """the 30 uint8 41 x 41 pinhole windows embedded in zero frames of 131 x 203 at seeded offsets, and the reference's kernel"""
    g = load_golden("pinholes.npz")
    rng = np.random.default_rng(459)
    H, W = EMBED
    frames = np.zeros((len(g["windows"]), H, W), np.uint8)
    for k, w in enumerate(g["windows"]):
        oy, ox = int(rng.integers(0, H - 41 + 1)), int(rng.integers(0, W - 41 + 1))
        frames[k, oy:oy + 41, ox:ox + 41] = w
    frames.setflags(write=False)
    host = session.psf_from_pinhole_images(list(frames))
    assert np.abs(host - g["psf_m"]).max() == 0.0  # the host form under this embedding gives the reference's bits
    return frames, g["psf_m"]


# ---- 1. reference parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_reference_parity(kind, golden):
    """psf within 1e-14 of the reference's own output: the window sums are exact integers, what remains is fewer than 36 + 49 + 4 roundings
    of 2^-53 on quantities <= 1.  Peaks equal np.argmax exactly (windows 3 and 16 hold two equal maxima each: the tie rule)."""
    frames, psf_m = golden
    psf, info = run(dev(frames, kind), kind)
    d = float(np.abs(psf - psf_m).max())
    print(f"{kind}: max |psf - psf_m| = {d:.3e}")
    assert np.array_equal(info[:, :2], argmax_rc(frames))
    assert info[:, 2].all()
    assert d <= 1e-14


# ---- 2. arg-max alone ---------------------------------------------------------------------------------------------------------------
ARG_SHAPE = {"u8": (151, 451), "f32": (101, 173), "f64": (83, 107)}  # odd H W, just past two chunks of 32 KiB: three workgroups, a ragged last


def _layout(ptr, k, HW, eb):
    """the arg-max kernel's split of frame k (csrc/srx_psf.hpp): per chunk (lo, first vector sample, first tail sample, hi)"""
    C, ve = psf_device.CHUNK_BYTES // eb, 16 // eb
    out = []
    for lo in range(0, HW, C):
        hi = min(lo + C, HW)
        head = min(((-(ptr + (k * HW + lo) * eb)) % 16) // eb, hi - lo)
        nvec = (hi - lo - head) // ve
        out.append((lo, lo + head, lo + head + nvec * ve, hi))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_argmax(kind):
    H, W = ARG_SHAPE[kind]
    HW, eb = H * W, EB[kind]
    C, ve = psf_device.CHUNK_BYTES // eb, 16 // eb
    assert 2 * C < HW < 3 * C and HW % 2 == 1
    rng = np.random.default_rng(7)
    lowv, topv = (200, 255) if kind == "u8" else (200.0, 250.5)
    REP = 4  # consecutive frame slots: the alignments a frame of odd H W takes
    names = ["first", "last", "chunk0_last", "chunk1_first", "head", "tail", "chunks_0_and_2", "one_vector"]
    if kind != "u8":
        names += ["negative", "zeros_minus_first", "zeros_plus_first"]
    N = REP * len(names) + 2
    x = torch.empty((N, H, W), dtype=TORCH_DT[kind], device=CUDA)
    a = rng.integers(0, int(lowv), (N, HW)).astype(NP_DT[kind])
    if kind != "u8":
        a += NP_DT[kind](0.25)
    seen = {"head": 0, "tail": 0, "chunk0_last_in_tail": 0}
    for ci, name in enumerate(names):
        for r in range(REP):
            k = ci * REP + r
            lay = _layout(x.data_ptr(), k, HW, eb)
            assert len(lay) == 3 and lay[2][3] - lay[2][0] < C
            f = a[k]
            if name == "first":
                f[0] = topv
            elif name == "last":
                f[HW - 1] = topv
            elif name == "chunk0_last":
                f[C - 1] = topv
                seen["chunk0_last_in_tail"] += lay[0][2] <= C - 1
            elif name == "chunk1_first":
                f[C] = topv
            elif name == "head":  # the last peeled sample in front of chunk 1's first vector (chunk 0's when chunk 1 has none)
                c = 1 if lay[1][1] > lay[1][0] else 0
                if lay[c][1] > lay[c][0]:
                    f[lay[c][1] - 1] = topv
                    seen["head"] += 1
                else:
                    f[lay[c][1]] = topv
            elif name == "tail":  # the first sample behind the last whole vector of the last chunk
                if lay[2][2] < HW:
                    f[lay[2][2]] = topv
                    seen["tail"] += 1
                else:
                    f[HW - 2] = topv
            elif name == "chunks_0_and_2":
                f[C - 5 - r] = f[2 * C + 3 + r] = topv
            elif name == "one_vector":  # two equal maxima in the same aligned 16 bytes
                v0 = lay[1][1] + 7 * ve
                f[v0 + ve - 1] = f[v0 + (ve - 2 if ve > 2 else 0)] = topv
            elif name == "negative":
                f[:] = -1.0 - f
                f[C + 11 + r] = -0.5
            elif name == "zeros_minus_first":
                f[:] = -1.0 - f
                f[C - 2 - r], f[C + 40] = -0.0, 0.0
            elif name == "zeros_plus_first":
                f[:] = -1.0 - f
                f[2 * C + 1 + r], f[2 * C + 90] = 0.0, -0.0
    # slot N - 2: random samples with many tied maxima (uint8: many 255s); slot N - 1: a constant frame
    a[N - 2] = rng.integers(0, 256, HW).astype(NP_DT[kind]) if kind == "u8" else rng.integers(0, 64, HW).astype(NP_DT[kind])
    a[N - 1] = 17
    assert seen["head"] >= 1 and seen["tail"] >= 1 and seen["chunk0_last_in_tail"] >= 1, seen
    a = a.reshape(N, H, W)
    x.copy_(torch.from_numpy(a))
    _, info = run(x, kind)
    want = argmax_rc(a)
    bad = [(k, names[k // REP] if k < REP * len(names) else "random/constant", tuple(info[k, :2]), tuple(want[k]))
           for k in range(N) if not np.array_equal(info[k, :2], want[k])]
    assert not bad, bad
    assert tuple(info[N - 1]) == (0, 0, 0)  # a constant frame: (0, 0), and a peak there is closer than reach to the border
    assert (a[N - 2] == a[N - 2].max()).sum() > 50


def test_argmax_ignores_nan():
    """Frames are documented NaN-free; the defined behaviour if they are not: a NaN never wins, an all-NaN frame reports (0, 0)."""
    H, W = ARG_SHAPE["f32"]
    for kind in ("f32", "f64"):
        a = np.full((3, H * W), 1.0, NP_DT[kind])
        a[0, ::3] = np.nan
        a[0, 0] = np.nan
        a[0, 9001] = 2.0
        a[1, :] = np.nan
        a[2, :] = np.nan
        a[2, H * W - 2] = -np.inf
        _, info = run(dev(a.reshape(3, H, W), kind), kind)
        assert tuple(info[0, :2]) == divmod(9001, W)
        assert tuple(info[1, :2]) == (0, 0)
        assert tuple(info[2, :2]) == divmod(H * W - 2, W)


# ---- 3. the drop rule ---------------------------------------------------------------------------------------------------------------
def _spot(H, W, r, c):
    f = np.zeros((H, W), np.uint8)
    f[r, c] = 200
    return f


def test_drop_rule(golden):
    H, W, reach = 40, 50, 9
    near = [(reach - 1, 25), (H - reach, 25), (20, reach - 1), (20, W - reach)]      # distance reach - 1 from one border each
    at = [(reach, reach), (H - reach - 1, W - reach - 1), (reach, W - reach - 1), (H - reach - 1, reach)]
    frames = np.stack([_spot(H, W, r, c) for r, c in near + at])
    for kind in KINDS:
        psf, info = run(dev(frames, kind), kind)
        assert np.array_equal(info[:, :2], np.array(near + at))
        assert info[:, 2].tolist() == [0] * 4 + [1] * 4
        assert np.isfinite(psf).all() and abs(psf.sum() - 1.0) < 1e-15
        # every frame dropped: all zeros from the library, FileNotFoundError from the wrapper (as the host form)
        psf0, info0 = run(dev(frames[:4], kind), kind)
        assert not info0[:, 2].any() and np.array_equal(psf0, np.zeros((7, 7)))
        with pytest.raises(FileNotFoundError, match="no usable pinhole image"):
            psf_device.estimate_psf(dev(frames[:4], kind))
    # one bad frame among the 30 golden ones leaves the kernel as it was (the device twin of test_psf_skips_peaks_near_the_edge)
    gf, psf_m = golden
    bad = np.zeros(EMBED, np.uint8)
    bad[2, 20] = 255
    base, _ = run(dev(gf, "u8"), "u8")
    psf, info = run(dev(np.concatenate([gf[:11], bad[None], gf[11:]]), "u8"), "u8")
    assert tuple(info[11]) == (2, 20, 0) and info[:, 2].sum() == 30
    assert np.array_equal(psf, base) and np.abs(psf - psf_m).max() <= 1e-14


# ---- 4. float frames against the host form --------------------------------------------------------------------------------------------
def _blobs(n, H, W, seed):
    """non-integer frames: a blob of peak >= 200 on a background <= 10 (cancellation in core - background stays small)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(n):
        cy, cx = rng.uniform(20, H - 20), rng.uniform(20, W - 20)
        s = rng.uniform(1.2, 2.0)
        out.append(rng.uniform(200, 240) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + rng.uniform(0, 10, (H, W)))
    return np.stack(out)


@pytest.mark.parametrize("halfwidth", [1, 3, 7])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_float_frames_match_host_form(kind, halfwidth):
    """Tolerance, derived: the n-term window sum and its division, the 36-term background mean, the side^2-term sum and the subtraction,
    clip, division and conversion -- fewer than n + 36 + side^2 + 4 roundings of 2^-53, each on a quantity <= max(core) relative to the
    clipped sum s.  Every sum is formed in numpy's own order (frame order for the mean over the stack, its eight-lane pairwise order for the
    two contiguous reductions), so in float64 arithmetic on the same values the result is the host form's, bit for bit -- which is how
    the window mean (it has no output of its own) is held to bit-identity."""
    n, H, W = 5, 67, 75
    frames = _blobs(n, H, W, 100 + halfwidth).astype(NP_DT[kind])
    host = session.psf_from_pinhole_images(list(frames), halfwidth=halfwidth)
    side, reach = 2 * halfwidth + 1, halfwidth + 6
    span = np.arange(-reach, reach + 1)
    wins = [f.astype(np.float64)[np.ix_(p[0] + span, p[1] + span)] for f, p in zip(frames, argmax_rc(frames))]
    core = np.stack(wins).mean(axis=0)[6:6 + side, 6:6 + side]
    edge = np.r_[0:3, side - 3:side]
    clipped = np.maximum(core - core[np.ix_(edge, edge)].mean(), 0.0)
    s = clipped.sum()
    assert core.max() >= 150 and np.array_equal(clipped / s, host)
    tol = 2.0 ** -53 * (n + 36 + side * side + 4) * max(1.0, core.max() / s)
    psf, info = run(dev(frames, kind), kind, halfwidth)
    d = float(np.abs(psf - host).max())
    print(f"{kind} halfwidth {halfwidth}: max |device - host| = {d:.3e}, tolerance {tol:.3e}")
    assert np.array_equal(info[:, :2], argmax_rc(frames)) and info[:, 2].all()
    assert d <= tol
    assert np.array_equal(psf, host), "same values, same order, float64: the device result must be the host form's bits"
    # the wrapper: the working precision for float frames, the kernel ready for ibp
    with api.precision_override(kind):
        k, peaks, used = psf_device.estimate_psf(list(frames), halfwidth=halfwidth, full=True)
    assert k.dtype == np.float64 and k.shape == (side, side) and np.array_equal(k, psf)
    assert np.array_equal(peaks, argmax_rc(frames)) and used.dtype == bool and used.all()


# ---- 5. memory contract -----------------------------------------------------------------------------------------------------------------
CONTRACT = T.ids(["srx_psf_estimate_u8-odd_byte", "srx_psf_estimate_f32-element_aligned", "srx_psf_estimate_f64-element_aligned"])


@pytest.mark.parametrize("case", CONTRACT)
def test_memory_contract(case, golden):
    """Guard bands around psf and info intact; the workspace poisoned with every pattern, the results the same and nothing written beyond
    ws_bytes; inputs unchanged; frames sliced one element off the 256-byte grid (uint8: an odd byte); a workspace one byte short or
    misaligned is SRX_E_WORKSPACE with nothing written; two calls give identical bits."""
    kind = case.split("-")[0].rsplit("_", 1)[1]
    gf, psf_m = golden
    frames = np.zeros((len(gf), 181, 203), np.uint8)  # two chunks of uint8, five of float32, nine of float64
    frames[:, 25:25 + EMBED[0]] = gf
    N, H, W = frames.shape
    x = T.put(dev(frames, kind), skip=1)
    assert x.data_ptr() % 16 == EB[kind]
    psf, info = T.out((7, 7), torch.float64), T.out((N, 3), torch.int32)
    need = need_bytes(kind, N, H, W, 3)

    def call(wp, wn):
        return entry(kind)(T.p(x), N, H, W, 3, T.p(psf.t), T.p(info.t), wp, wn, api._stream())

    first = T.contract(call, [psf, info], need, [x])
    assert np.abs(first[0].cpu().numpy() - psf_m).max() <= 1e-14
    assert np.array_equal(first[1].cpu().numpy()[:, :2], argmax_rc(frames))
    ws = MG.Guarded(need, CUDA)
    assert call(ctypes.c_void_p(ws.ptr), ctypes.c_size_t(need)) == _lib.OK
    torch.cuda.synchronize()
    assert torch.equal(psf.t, first[0]) and torch.equal(info.t, first[1])
    # info may be NULL
    psf.fill(MG.POISON_NAN)
    assert entry(kind)(T.p(x), N, H, W, 3, T.p(psf.t), None, ctypes.c_void_p(ws.ptr), ctypes.c_size_t(need), api._stream()) == _lib.OK
    torch.cuda.synchronize()
    psf.check("info = NULL: psf")
    ws.check("info = NULL: workspace")
    assert torch.equal(psf.t, first[0])


# ---- 6. files to kernel -----------------------------------------------------------------------------------------------------------------
def test_files_to_kernel(tmp_path, golden, g_c1):
    from PIL import Image
    gf, _ = golden
    for i in range(3):
        d = tmp_path / f"sweep{i}"
        d.mkdir()
        Image.fromarray(gf[i]).save(str(d / "pos4_(0,0).png"))
    (tmp_path / "sweep3").mkdir()                       # a sweep without the file
    (tmp_path / "notes.txt").write_text("not a sweep")  # a stray file
    host = session.load_measured_psf(str(tmp_path))
    got = session.load_measured_psf_device(str(tmp_path))
    assert got.dtype == np.float64 and got.shape == (7, 7)
    assert np.abs(got - host).max() <= 1e-14
    assert np.array_equal(got, host)  # uint8 frames: exact window sums, the same operations in the same order behind them
    lr, sh = list(g_c1["lr_meas"]), g_c1["shifts_meas"]
    init = api.shift_and_add(lr, sh, 2)
    a, ea = api.ibp(lr, sh, got, init, 2, 5, 0.5, verbose=False)
    b, eb = api.ibp(lr, sh, host, init, 2, 5, 0.5, verbose=False)
    assert np.array_equal(a, b) and np.array_equal(np.asarray(ea), np.asarray(eb))
    with pytest.raises(FileNotFoundError):
        session.load_measured_psf_device(str(tmp_path / "sweep3"))
