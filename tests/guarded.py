"""A guarded arena for footprint tests: buffers of an EXACT byte length inside poisoned guard bands.

Not collected by pytest (no test_ prefix); tests/test_guarded_host.py proves on the CPU that it can fail, and
tests/test_gpu_footprint.py hands its pointers to the C ABI.  It works on any torch device.

    a = Arena(device, "nan")
    x = a.buf("X", nbytes, data=X)                  # an input: real data inside poisoned guards
    y = a.buf("Y", nbytes)                          # an output / scratch: every byte poisoned
    w = a.buf("workspace", nbytes, zero_head=256)   # ... except a status block that must be zero
    a.commit()                                      # one uint8 tensor; lays out, fills, copies the inputs in
    call(x.ptr, y.ptr, w.ptr); synchronise
    a.check()                                       # {} or {name: {"front" / "back": (first, last, count)}}
    y.unwritten(4)                                  # elements of the output that still hold the poison

Layout: every buffer starts on a 256-byte boundary (what a fresh torch allocation gives; `offset` moves it off that on
purpose) with at least GUARD bytes of guard in front, and behind it the bytes up to the next 256-byte boundary plus at
least GUARD more.  All of it is one allocation of our own, so that a small overrun is SEEN and never faults.
The fill is a function of the absolute arena offset and the seed alone: two arenas laid out alike hold the same bytes.
"""
from __future__ import annotations

import functools

import torch

GUARD = 4096
ALIGN = 256
NAN_WORD = 0x7FC07FC0            # a NaN as fp32 and, half by half, as fp16 and as bf16
PERIOD = 1 << 22                 # words after which the "finite" pattern repeats (16 MiB)
FILLS = ("zero", "finite", "nan")   # the order the tests use them in


def _rup(x: int, a: int) -> int:
    return (x + a - 1) // a * a


@functools.lru_cache(maxsize=8)
def _pattern(fill: str, seed: int) -> torch.Tensor:
    """PERIOD words of the fill on the CPU (large arenas repeat it: the host generates it once per fill and seed)."""
    n = PERIOD
    if fill == "zero":
        return torch.zeros(n, dtype=torch.int32)
    if fill == "nan":
        return torch.full((n,), NAN_WORD, dtype=torch.int32)
    if fill == "finite":
        # mixed sign, magnitudes 1e-4 .. 1e4; the high half of such a word is an ordinary bf16 and (exponent bits 30..26
        # not all ones) an ordinary fp16; the low half is made one too by clearing bit 10 wherever its bits 14..10 are
        # all ones (an fp16 inf / NaN, and a fortiori the bf16 one: bits 14..7) -- a change of 2^-13 relative
        g = torch.Generator().manual_seed(0x5EED + seed)
        v = torch.pow(10.0, torch.rand(n, generator=g) * 8.0 - 4.0)
        v = torch.where(torch.rand(n, generator=g) < 0.5, -v, v).to(torch.float32)
        w = v.view(torch.int32)
        return torch.where((w & 0x7C00) == 0x7C00, w & ~0x0400, w)
    raise ValueError("unknown fill %r (one of %s)" % (fill, ", ".join(FILLS)))


def fill_bytes(fill: str, nbytes: int, device, seed: int = 0) -> torch.Tensor:
    """nbytes (a multiple of 4) of the fill pattern as a uint8 tensor on `device`.  Generated on the CPU and copied, so the
    bytes do not depend on the device's random number generator."""
    assert nbytes % 4 == 0
    total = nbytes // 4
    w = _pattern(fill, seed)
    w = w.repeat((total + PERIOD - 1) // PERIOD)[:total] if total > PERIOD else w[:total]
    return w.contiguous().view(torch.uint8).to(device, copy=True)


class Buf:
    """One named buffer of the arena: [start, start + nbytes) of its uint8 tensor."""

    def __init__(self, arena, name, nbytes, data, zero_head, offset):
        self.arena, self.name, self.nbytes, self.data, self.zero_head, self.offset = arena, name, nbytes, data, zero_head, offset
        self.start = self.guard_lo = self.guard_hi = None

    @property
    def ptr(self) -> int:
        return self.arena.mem.data_ptr() + self.start

    def bytes(self) -> torch.Tensor:
        return self.arena.mem[self.start:self.start + self.nbytes]

    def view(self, dtype, shape=None) -> torch.Tensor:
        """The buffer as a tensor of `dtype` (a view when the start is aligned to the element, else a copy)."""
        b = self.bytes()
        item = torch.empty((), dtype=dtype).element_size()
        assert self.nbytes % item == 0, (self.name, self.nbytes, dtype)
        t = b.view(dtype) if (self.start % item == 0 and b.data_ptr() % item == 0) else b.clone().view(dtype)
        return t if shape is None else t.reshape(shape)

    def host(self) -> torch.Tensor:
        """The buffer's bytes, copied to the CPU."""
        return self.bytes().cpu().clone()

    def write(self, src: torch.Tensor) -> None:
        """Overwrite the buffer with the bytes of `src` (a contiguous tensor of exactly nbytes)."""
        s = src.contiguous().reshape(-1).view(torch.uint8)
        assert s.numel() == self.nbytes, (self.name, s.numel(), self.nbytes)
        self.bytes().copy_(s.to(self.arena.device))

    def poison(self) -> None:
        """Every byte back to the arena's fill (the zero head stays zero): a scratch buffer between two calls."""
        self.bytes().copy_(self.arena.pristine[self.start:self.start + self.nbytes])

    def unwritten(self, itemsize: int) -> int:
        """Elements of `itemsize` bytes whose bytes equal what the buffer held at commit().  For an output under the
        "finite" and "nan" fills: the poison that survived the call."""
        assert self.nbytes % itemsize == 0
        now = self.bytes().reshape(-1, itemsize)
        was = self.arena.pristine[self.start:self.start + self.nbytes].reshape(-1, itemsize)
        return int((now == was).all(dim=1).sum())


class Arena:
    def __init__(self, device, fill: str, seed: int = 0):
        if fill not in FILLS:
            raise ValueError("unknown fill %r" % (fill,))
        self.device, self.fill, self.seed = torch.device(device), fill, seed
        self.bufs = {}
        self.mem = self.pristine = None
        self._cursor = 0

    def buf(self, name: str, nbytes: int, data: torch.Tensor = None, zero_head: int = 0, offset: int = 0) -> Buf:
        """Reserve `nbytes` (exact, >= 1).  data: the bytes it starts with (an input, or scratch left dirty by someone
        else); None: the fill.  zero_head: that many leading bytes are zero whatever the fill (the status block).
        offset: bytes past the 256-byte boundary at which the buffer starts (alignment tests)."""
        assert self.mem is None, "buf() after commit()"
        assert name not in self.bufs and nbytes >= 1 and 0 <= offset < ALIGN and zero_head <= nbytes
        b = Buf(self, name, int(nbytes), data, zero_head, offset)
        b.guard_lo = self._cursor
        b.start = _rup(self._cursor + GUARD, ALIGN) + offset
        b.guard_hi = _rup(b.start + b.nbytes, ALIGN) + GUARD
        self._cursor = b.guard_hi
        self.bufs[name] = b
        return b

    def commit(self) -> "Arena":
        total = _rup(self._cursor + GUARD, ALIGN)
        self.mem = fill_bytes(self.fill, total, self.device, self.seed)
        for b in self.bufs.values():
            if b.data is not None:
                b.write(b.data)
                b.data = None
            if b.zero_head:
                self.mem[b.start:b.start + b.zero_head] = 0
        self.pristine = self.mem.clone()
        return self

    def __getitem__(self, name: str) -> Buf:
        return self.bufs[name]

    def _changed(self, lo: int, hi: int, origin: int):
        diff = (self.mem[lo:hi] != self.pristine[lo:hi]).nonzero()
        if diff.numel() == 0:
            return None
        return (int(diff[0]) + lo - origin, int(diff[-1]) + lo - origin, int(diff.numel()))

    def check(self) -> dict:
        """Per buffer whose guard bands changed since commit(): {"front": (first, last, count), "back": (...)} with the
        offsets in bytes from the buffer's first byte (front: negative; back: >= its length).  {} = all intact.
        Synchronise the device before calling."""
        report = {}
        for b in self.bufs.values():
            r = {}
            front = self._changed(b.guard_lo, b.start, b.start)
            back = self._changed(b.start + b.nbytes, b.guard_hi, b.start)
            if front:
                r["front"] = front
            if back:
                r["back"] = back
            if r:
                report[b.name] = r
        return report
