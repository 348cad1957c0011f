"""Poisoned, guarded buffers for the tests of kernels that write into caller memory.

A plain helper module (no pytest hooks).  guarded() allocates ONE parent uint8 tensor laid out as

    [ front band | interior | back band ]

fills every byte of it with `fill` and hands out the interior as a tensor of the requested dtype.
A kernel that leaves an output element unwritten leaves the poison there (0xFF: a NaN pattern in
every float type and -1 in every integer type; 0x00: zeros, for a kernel that relies on garbage
being nonzero), and a store that lands just outside the interior changes a band, which check()
reports with the offset of the first changed byte relative to the interior.

The bands are BAND = 4096 bytes each.  That is the check's reach, not a measurement: a stray
store further away than 4096 bytes from the interior is not seen.

The interior starts on a 256-byte boundary, the alignment a device allocation's base has, so that
no kernel takes another alignment branch on a guarded buffer than on a plain one (the front band
is padded at its start for that; the padding is poisoned and checked like the band).  A
zero-length interior still gets both bands.  Works on CPU tensors as well.
"""
from __future__ import annotations

import numpy as np

BAND = 4096
ALIGN = 256


def torch_dtype(dtype):
    """The torch dtype of a numpy dtype, a dtype name or a torch dtype (the names agree)."""
    import torch
    if isinstance(dtype, torch.dtype):
        return dtype
    return getattr(torch, np.dtype(dtype).name)


class Guarded:
    """One guarded buffer: `.t` the interior (a tensor of the dtype asked for), `.nbytes` its
    size, `.fill` the poison byte, `.parent` the uint8 tensor that holds bands and interior."""

    def __init__(self, shape, dtype, fill=0xFF, device="cpu", name=""):
        import torch
        tdt = torch_dtype(dtype)
        item = torch.empty(0, dtype=tdt).element_size()
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        shape = tuple(int(s) for s in shape)
        count = int(np.prod(shape, dtype=np.int64)) if shape else 1
        self.nbytes = count * item
        self.fill = int(fill) & 0xFF
        self.name = name
        # the interior ends on the element size, so the back band starts right behind it
        self.parent = torch.full((BAND + ALIGN + self.nbytes + BAND,), self.fill, dtype=torch.uint8, device=device)
        base = self.parent.data_ptr()
        self.front = (-(base + BAND)) % ALIGN + BAND           # bytes in front of the interior (>= BAND)
        self.back = self.front + self.nbytes                   # first byte of the back band
        self.t = self.parent[self.front:self.back].view(tdt).view(shape)
        self.ptr = base + self.front                           # (an empty tensor reports no address of its own)
        assert self.ptr % ALIGN == 0 and (self.nbytes == 0 or self.t.data_ptr() == self.ptr)

    def data_ptr(self):
        """Address of the interior's first byte, also for an empty interior."""
        return self.ptr

    def bytes(self):
        """The interior as uint8 (a view)."""
        return self.parent[self.front:self.back]

    def refill(self):
        """Poison the whole parent again."""
        self.parent.fill_(self.fill)

    def check(self, what=""):
        """Both bands still hold `fill` in every byte (the front band with its alignment padding;
        BAND bytes behind the interior)."""
        what = what or self.name or "buffer"
        for band, lo, hi in (("front", 0, self.front), ("back", self.back, self.back + BAND)):
            bad = (self.parent[lo:hi] != self.fill).nonzero()
            if bad.numel():
                first = int(bad[0, 0]) + lo - self.front
                got = int(self.parent[first + self.front])
                raise AssertionError(f"{what}: {band} guard band changed, {bad.shape[0]} bytes, first at byte offset "
                                     f"{first} from the interior's start (interior: {self.nbytes} bytes), "
                                     f"0x{got:02x} where the fill is 0x{self.fill:02x}")


def guarded(nbytes_or_shape, dtype="uint8", fill=0xFF, device="cpu", name=""):
    """A poisoned buffer of `nbytes_or_shape` elements of `dtype` (an int or a shape) between two
    4096-byte guard bands, every byte of all three set to `fill`; see the module docstring."""
    return Guarded(nbytes_or_shape, dtype, fill, device, name)
