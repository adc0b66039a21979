"""Output arrays with guard regions, for calling the C-ABI the way a C or Rust caller does: an
array of exactly `count` elements that the library gets a raw pointer to, with GUARD_BYTES of a
fixed byte pattern directly before and after it.  check() asserts that neither guard changed,
i.e. that the call wrote nothing outside the capacity it was given.  Host memory only.
"""
import numpy as np

GUARD_BYTES = 256   # a multiple of 64: the array inside keeps the allocation's alignment
GUARD_BYTE = 0xA5   # the guards' pattern
FILL_BYTE = 0xEE    # the array's own bytes before the call (no offset, status or record is made of these)


class Guarded:
    """`count` elements of `dtype` between two guards.  .a is the array (a view into the guarded
    allocation), .ptr its address for ctypes."""

    def __init__(self, count, dtype, name="array"):
        self.name, self.dtype = name, np.dtype(dtype)
        self.nbytes = int(count) * self.dtype.itemsize
        self.raw = np.full(2 * GUARD_BYTES + self.nbytes, GUARD_BYTE, dtype=np.uint8)
        body = self.raw[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        body[:] = FILL_BYTE
        self.a = body.view(self.dtype)
        assert self.a.ctypes.data % 8 == 0

    @property
    def ptr(self):
        return self.raw.ctypes.data + GUARD_BYTES

    def damaged(self):
        """Byte offsets relative to the array's start (negative: before it; >= nbytes: past its end)
        of every guard byte that changed."""
        lo = np.nonzero(self.raw[:GUARD_BYTES] != GUARD_BYTE)[0] - GUARD_BYTES
        hi = np.nonzero(self.raw[GUARD_BYTES + self.nbytes:] != GUARD_BYTE)[0] + self.nbytes
        return [int(x) for x in lo] + [int(x) for x in hi]

    def check(self):
        bad = self.damaged()
        assert not bad, (f"{self.name}[{len(self.a)}] ({self.nbytes} bytes): {len(bad)} byte(s) written outside "
                         f"the array, at byte offsets {bad[:8]}")

    def untouched(self):
        """The array itself still holds only its fill pattern."""
        return bool((self.raw[GUARD_BYTES:GUARD_BYTES + self.nbytes] == FILL_BYTE).all())

    def bytes(self, count=None):
        """The first `count` elements (default: all) as bytes."""
        return (self.a if count is None else self.a[:count]).tobytes()


class GuardedSet(dict):
    """The guarded arrays of one call, by name; .rc is the call's return code."""
    rc = None

    def add(self, name, count, dtype):
        self[name] = Guarded(count, dtype, name)
        return self[name].ptr

    def check(self):
        for g in self.values():
            g.check()
        return self
