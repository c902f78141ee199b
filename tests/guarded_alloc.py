"""Guard bands and poisoned surroundings for the engine's device allocations.

Every device allocation of the launch sequence goes through `PlaneSweepEngine.empty`.  `guarded(eng, fill_byte)` replaces
it on the INSTANCE for the duration of a `with` block: each request becomes one flat uint8 buffer of
BAND + payload + BAND bytes obtained through the original `empty` (so a forward that is being recorded keeps the buffer
alive exactly as it keeps a plain tensor), filled bytewise with `fill_byte`, and the caller gets the typed contiguous view
of the payload.  On exit the bands of every allocation must still hold the fill byte.

Two fills tell three kinds of error apart without a tolerance:
  0xFF  every float word is a NaN, every 32-bit tag word 0xFFFFFFFF
  0x7B  every float is ~1.3e36, finite
An element nobody writes differs between the two; a read of unwritten or foreign memory that reaches a result differs
from the plain run (or is NaN under 0xFF); a store outside the tensor breaks a band.

BAND = 64 KiB + 16 bytes: the payload is 16-byte aligned and NOT 32-byte aligned (the alignment the library's header
promises to need, and what a batch slice inside the engine has).  64 KiB is several times the largest plausible overrun at
test shapes (15 tile rows x 136 columns x 4 B ~ 8 KB): a condition, not a measurement -- a wrong store must land in memory
the test owns.
"""
import contextlib

import torch

BAND = (64 << 10) + 16
POISON_NAN = 0xFF
POISON_FINITE = 0x7B


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


class _Allocation:
    __slots__ = ("base", "nbytes", "shape", "dtype", "order", "what")

    def __init__(self, base, nbytes, shape, dtype, order, what):
        self.base, self.nbytes, self.shape, self.dtype, self.order, self.what = base, nbytes, shape, dtype, order, what

    def bands(self):
        return self.base[:BAND], self.base[BAND + self.nbytes:]

    def describe(self):
        return f"{self.what} #{self.order} shape {tuple(self.shape)} dtype {self.dtype}"


class Guard:
    """The allocations made under one `guarded` block, in request order."""

    def __init__(self, alloc, fill_byte):
        assert 0 <= int(fill_byte) <= 0xFF
        self._alloc, self.fill = alloc, int(fill_byte)
        self.allocations = []

    def _carve(self, shape, dtype, device, what):
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        nbytes = _numel(shape) * torch.empty((), dtype=dtype).element_size()
        base = self._alloc((BAND + nbytes + BAND,), dtype=torch.uint8, device=device)
        assert base.dtype == torch.uint8 and base.is_contiguous() and base.numel() == 2 * BAND + nbytes
        assert base.data_ptr() % 32 == 0, "the allocator's own alignment is the premise of the 16-byte-only payload"
        base.fill_(self.fill)
        self.allocations.append(_Allocation(base, nbytes, shape, dtype, len(self.allocations), what))
        return base[BAND:BAND + nbytes].view(dtype).view(shape)

    def empty(self, shape, dtype=torch.float32, device=None, **_):
        return self._carve(shape, dtype, device, "allocation")

    def poisoned(self, tensor):
        """`tensor` copied into a payload of its own (its bands are checked with the others)."""
        view = self._carve(tuple(tensor.shape), tensor.dtype, tensor.device, "input")
        view.copy_(tensor)
        return view

    def damage(self):
        """[(allocation, first damaged byte offset relative to the payload)] of the allocations whose bands changed."""
        if not self.allocations:
            return []
        if any(a.base.is_cuda for a in self.allocations):
            torch.cuda.synchronize()
        flags = torch.stack([(lo != self.fill).any() | (hi != self.fill).any()
                             for lo, hi in (a.bands() for a in self.allocations)]).cpu().tolist()
        out = []
        for a, bad in zip(self.allocations, flags):
            if not bad:
                continue
            lo, hi = a.bands()
            before = (lo != self.fill).nonzero()
            if before.numel():
                out.append((a, int(before[0, 0]) - BAND))
            else:
                out.append((a, a.nbytes + int((hi != self.fill).nonzero()[0, 0])))
        return out

    def check(self):
        bad = self.damage()
        assert not bad, "guard band damaged (fill 0x%02X): " % self.fill + "; ".join(
            f"{a.describe()}: first damaged byte at payload offset {off:+d} (payload is {a.nbytes} bytes)" for a, off in bad)


@contextlib.contextmanager
def guarded(eng, fill_byte):
    """Route `eng.empty` through guard-banded, poisoned buffers; restore it on exit (also when the body raises) and, after
    a body that ended normally, synchronise and assert that every band still holds the fill byte."""
    had = "empty" in vars(eng)
    previous = vars(eng).get("empty")
    guard = Guard(eng.empty, fill_byte)          # the bound original: a recording forward keeps the base buffer
    eng.empty = guard.empty
    try:
        yield guard
    finally:
        if had:
            eng.empty = previous
        else:
            del eng.empty
    guard.check()


def poisoned(tensor, fill_byte=POISON_NAN):
    """A contiguous copy of `tensor` inside a poisoned buffer of its own: NaN (0xFF) surroundings, 16-byte-only alignment."""
    def alloc(shape, dtype, device):
        return torch.empty(shape, dtype=dtype, device=device)
    return Guard(alloc, fill_byte).poisoned(tensor)


def bits_equal(a, b):
    """Equality of the stored bits: NaN payloads and the sign of zero count."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
