"""Guard bands, poisoned scratch and intact inputs: the checker behind tests/test_gpu_memory_contract.py (its own logic is tested on CPU
tensors by tests/test_memguard_host.py).  A plain helper module like ssim_oracle.py: no fixtures, nothing registered.

include/srx.h promises that a call writes its outputs and its workspace and nothing else, that the workspace may hold anything on
entry, and that inputs are never written.  Buffers from torch.empty cannot show a violation: the caching allocator rounds sizes up and
hands out slices of large blocks (a store past the end lands in memory the process owns, compared by nobody), returns the same block
to the next call of the same size (a read of an unwritten workspace word sees the previous call's correct leftovers), and an output
element nobody wrote keeps a plausible pixel.  So:

  Guarded       ONE uint8 allocation  guard | payload | guard.  The payload starts on a 256-byte boundary (srx.h's workspace alignment)
                and is exactly `nbytes` long -- the byte behind it is guard, not padding.  Both guards hold a position-dependent pattern,
                (131 i + 7) & 0xFF, so a stray run of zeros, of 0xFF or of image data all differ from it; check() reports the first and
                the last damaged byte as offsets relative to the payload (negative: in front of it; >= nbytes: behind it), which is what
                points at the kernel and the row.
  poisons       the payload of every output and of the workspace is filled before a call: 0xFF bytes (a NaN in float32 and float64, -1 in
                int32), 0x00 bytes, and 0x4B bytes (1.3e7 in float32, 3.0e54 in float64: finite garbage).
  run_poisoned  one run per poison; after each: status, guards, inputs bit-identical to their clones, outputs bit-identical to the first
                run's and finite.  Bit-identity ACROSS poisons needs no tolerance and catches both an output element nobody wrote and a
                read of uninitialised workspace that reaches a result (NaN * 0 is not 0).

Guard size: 1 MiB on each side.  That is a condition, not a measurement.  The tests exist to DETECT a silent overrun inside memory they own,
never to make the device fault, so a guard must be larger than the farthest a single mis-indexed row or tile of the shapes used can reach
beyond its buffer: the widest plane row in tests/test_gpu_memory_contract.py is below 8 KiB (577 float64 columns plus two 12-sample pads:
4.8 KiB), and the largest tile any kernel holds is a 256 x 256 patch of 8-byte elements = 512 KiB.  One row or one whole tile too far, in
either direction, therefore still lands in the guard (1 MiB >= 512 KiB + 8 KiB) and is reported instead of reaching someone else's tensor.
"""
import torch

GUARD_BYTES = 1 << 20
ALIGN = 256  # srx.h: the workspace pointer's alignment

POISON_NAN = 0xFF      # float32 / float64 NaN, int32 -1
POISON_ZERO = 0x00
POISON_GARBAGE = 0x4B  # float32 1.3e7, float64 3.0e54: finite, far from any pixel
POISONS = (POISON_NAN, POISON_ZERO, POISON_GARBAGE)
# integer outputs (uint8 images): two complementary bit patterns instead
POISON_INT_A = 0xA5
POISON_INT_B = 0x5A
INT_POISONS = (POISON_INT_A, POISON_INT_B)

_pattern_cache = {}


def pattern(n, device):
    """(131 i + 7) & 0xFF for i in [0, n) as uint8 on `device`"""
    key = str(device)
    p = _pattern_cache.get(key)
    if p is None or p.numel() < n:
        m = max(n, GUARD_BYTES + ALIGN)
        p = ((torch.arange(m, dtype=torch.int64, device=device) * 131 + 7) & 0xFF).to(torch.uint8)
        _pattern_cache[key] = p
    return p[:n]


class Guarded:
    """guard | payload (`nbytes`, 256-byte aligned, exact) | guard in one allocation.  `t`: a typed view of the payload (tensor()),
    `preset`: what `t` holds when a run starts instead of poison (an output that doubles as an input: hr_out == hr_init)."""

    def __init__(self, nbytes, device, poison=POISON_NAN, guard_bytes=GUARD_BYTES):
        nbytes = int(nbytes)
        if nbytes < 0:
            raise ValueError("nbytes must not be negative")
        self.nbytes, self.device = nbytes, torch.device(device)
        self.raw = torch.empty(guard_bytes + ALIGN + nbytes + guard_bytes, dtype=torch.uint8, device=self.device)
        self.off = guard_bytes + (-(self.raw.data_ptr() + guard_bytes)) % ALIGN
        self.front, self.payload, self.back = self.raw[:self.off], self.raw[self.off:self.off + nbytes], self.raw[self.off + nbytes:]
        self.t, self.preset, self.poison, self.skip_bytes = None, None, poison, 0
        self.front.copy_(pattern(self.front.numel(), self.device))
        self.back.copy_(pattern(self.back.numel(), self.device))
        self.payload.fill_(poison)

    @classmethod
    def tensor(cls, shape, dtype, device, skip=0, poison=POISON_NAN):
        """A Guarded whose payload is exactly `skip` elements of slack plus a contiguous tensor of `shape` / `dtype` (`.t`).  skip = 0: `.t`
        starts on the 256-byte boundary and ends where the guard begins; skip = 1: a pointer that is only element aligned."""
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            numel *= s
        isz = torch.empty((), dtype=dtype).element_size()
        g = cls((skip + numel) * isz, device, poison)
        g.t = g.payload[skip * isz:].view(dtype).view(shape)
        g.skip_bytes = skip * isz
        return g

    @property
    def ptr(self):
        return self.payload.data_ptr()

    def view(self, dtype, shape):
        """the first prod(shape) elements of the payload as a tensor of `dtype`"""
        isz = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= int(s)
        return self.payload[:numel * isz].view(dtype).view(tuple(shape))

    def fill(self, poison):
        self.poison = poison
        self.payload.fill_(poison)
        if self.preset is not None:
            self.t.copy_(self.preset)

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def damage(self):
        """None, or (first, last) damaged guard byte as offsets relative to the payload's first byte"""
        self._sync()
        bad = []
        for g, base in ((self.front, -self.front.numel()), (self.back, self.nbytes)):
            ne = g != pattern(g.numel(), self.device)
            if bool(ne.any()):
                idx = ne.nonzero().flatten()
                bad += [base + int(idx[0]), base + int(idx[-1])]
        return (min(bad), max(bad)) if bad else None

    def check(self, name="buffer"):
        d = self.damage()
        assert d is None, (f"{name}: guard damaged, first byte at payload offset {d[0]}, last at {d[1]} "
                           f"(payload is [0, {self.nbytes}); negative = in front of it)")
        if self.t is not None and self.skip_bytes:
            slack = self.payload[:self.skip_bytes]
            assert bool((slack == self.poison).all()), f"{name}: the slack in front of an element-aligned tensor was written"

    def untouched(self):
        """the whole payload still holds the poison it was filled with (a refused call stored nothing)"""
        self._sync()
        return self.preset is None and bool((self.payload == self.poison).all())


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8).clone()


def run_poisoned(call, outputs, workspace=(), inputs=(), poisons=POISONS, ok_status=0):
    """call() -> status, once per poison, with every Guarded of `outputs` (each with a typed view `.t`) and `workspace` freshly poisoned.
    After each run: status == ok_status; every guard intact; every tensor of `inputs` torch.equal to the clone taken before the run;
    every output bit-identical to the first run's; floating-point outputs finite.  Returns clones of the first run's outputs."""
    outputs, workspace, inputs = list(outputs), list(workspace), list(inputs)
    first_bytes, first = None, None
    for poison in poisons:
        for g in outputs + workspace:
            g.fill(poison)
        before = [x.clone() for x in inputs]
        status = call()
        for g in outputs + workspace:
            g._sync()
        assert status == ok_status, f"poison 0x{poison:02X}: status {status}, expected {ok_status}"
        for i, g in enumerate(outputs):
            g.check(f"poison 0x{poison:02X}: output {i}")
        for i, g in enumerate(workspace):
            g.check(f"poison 0x{poison:02X}: workspace {i}")
        for i, (x, c) in enumerate(zip(inputs, before)):
            assert torch.equal(x, c), f"poison 0x{poison:02X}: input {i} was modified"
        got = [_bytes(g.t) for g in outputs]
        for i, g in enumerate(outputs):
            if g.t.is_floating_point():
                assert bool(torch.isfinite(g.t).all()), f"poison 0x{poison:02X}: output {i} is not finite (an element nobody wrote, or poison read from the workspace)"
        if first_bytes is None:
            first_bytes, first = got, [g.t.clone() for g in outputs]
        else:
            for i, (a, b) in enumerate(zip(first_bytes, got)):
                if not torch.equal(a, b):
                    ne = (a != b).nonzero().flatten()
                    raise AssertionError(f"poison 0x{poison:02X}: output {i} differs from the run with poison 0x{poisons[0]:02X} "
                                         f"({int(ne.numel())} bytes, first at byte {int(ne[0])}, last at byte {int(ne[-1])}): "
                                         "the result depends on what the buffers held before the call")
    return first
