"""Guard bands and poisoned contents for the buffers a C ABI call writes (tests/test_hip_buffer_contracts.py).

The library owns no memory: every workspace, activation, output and gradient buffer is the caller's, sized by a *_bytes query or
by the extent include/nrms_hip.h states.  A callee may touch those bytes only, and may assume nothing about what a workspace
holds on entry.  Guarded(nbytes, dtype, poison) is ONE uint8 device allocation

    [ band | nbytes (the buffer) | band ]

whose middle part is handed to the library.  Both bands hold GUARD; assert_intact compares them with that pattern on the
device.  Each band is at least as long as the buffer and never shorter than 64 KiB, so an overrun that grows with the shape (one
more row, one more block total per 1 024 ids, one more tile) lands in memory this test owns: nothing here can fault the device.

GUARD is one byte repeated (period 1), different from every poison, so a store of 4 or 8 bytes of any plausible value -- a
float, an index, a count, -1, 0, NaN -- changes at least one byte of it.  The poisons are what a recycled block may hold:
0xFF (NaN as float / half, -1 as int32 / int64), 0x00, 0x7F (3.39e38 as float, a large positive integer)."""
import ctypes as C

import numpy as np
import torch

GUARD = 0xA5
POISONS = (0xFF, 0x00, 0x7F)
MIN_BAND = 64 * 1024
ALIGN = 256

assert GUARD not in POISONS


class Guarded:
    def __init__(self, nbytes, dtype=torch.uint8, poison=0xFF, device="cuda"):
        nbytes = int(nbytes)
        item = torch.empty(0, dtype=dtype).element_size()
        assert nbytes >= 0 and nbytes % item == 0, (nbytes, dtype)
        assert poison is None or poison in POISONS
        self.nbytes, self.dtype = nbytes, dtype
        want = max(MIN_BAND, (nbytes + ALIGN - 1) // ALIGN * ALIGN)
        self.raw = torch.full((want + ALIGN + nbytes + want,), GUARD, dtype=torch.uint8, device=device)
        self.lo = want + (-(self.raw.data_ptr() + want)) % ALIGN            # the buffer's first byte: 256-byte aligned
        self.hi = self.lo + nbytes
        assert (self.raw.data_ptr() + self.lo) % ALIGN == 0 and self.lo >= want and self.raw.numel() - self.hi >= want
        self.bytes = self.raw[self.lo:self.hi]
        self.view = self.bytes.view(dtype)                                   # zero-length for a zero-byte query
        self.fill(0x00 if poison is None else poison)

    @property
    def ptr(self):
        """Device address of the buffer (of its zero bytes, between the bands, if the query returned 0)."""
        return C.c_void_p(self.raw.data_ptr() + self.lo)

    def fill(self, byte):
        self.bytes.fill_(byte)
        return self

    def zero(self):
        """For buffers the header documents as accumulated or caller-initialised."""
        return self.fill(0x00)

    def set(self, array):
        """Caller-initialised contents (a tensor or an array of this buffer's dtype and size)."""
        t = torch.as_tensor(array).to(self.raw.device).contiguous()
        assert t.dtype == self.dtype and t.numel() == self.view.numel(), (t.dtype, t.numel(), self.dtype, self.view.numel())
        self.view.copy_(t.reshape(-1))
        return self

    def snapshot(self):
        return self.bytes.clone()

    def unchanged_since(self, snap):
        return torch.equal(self.bytes, snap)

    def numpy(self, shape=None):
        a = self.view.cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def assert_intact(self, name):
        """Both bands still hold GUARD.  Otherwise: which side, the first and last overwritten byte as offsets from the
        buffer's END (before the buffer: negative, counted from its start), and how many bytes differ."""
        bad = []
        for side, band, origin in (("before", self.raw[:self.lo], self.lo), ("after", self.raw[self.hi:], 0)):
            if bool((band == GUARD).all()):
                continue
            at = torch.nonzero(band != GUARD).flatten()
            first, last, n = int(at[0]) - origin, int(at[-1]) - origin, int(at.numel())
            if side == "after":
                bad.append("%d byte(s) overwritten AFTER the buffer, at offsets +%d .. +%d past its end" % (n, first, last))
            else:
                bad.append("%d byte(s) overwritten BEFORE the buffer, at offsets %d .. %d from its start" % (n, first, last))
        assert not bad, "%s (%d bytes, %s): %s" % (name, self.nbytes, str(self.dtype).replace("torch.", ""), "; ".join(bad))


class Pool:
    """The guarded buffers of one call sequence: intact(after) checks every band."""

    def __init__(self, poison):
        self.poison = poison
        self.bufs = {}

    def new(self, name, nbytes, dtype=torch.uint8, init=None):
        """init None: poisoned; 'zero': zeroed (accumulated / caller-initialised buffers); anything else: those contents."""
        g = Guarded(nbytes, dtype, None if init is not None else self.poison)
        if init is not None and not (isinstance(init, str) and init == "zero"):
            g.set(init)
        assert name not in self.bufs, name
        self.bufs[name] = g
        return g

    def elems(self, name, n, dtype=torch.float32, init=None):
        return self.new(name, int(n) * torch.empty(0, dtype=dtype).element_size(), dtype, init)

    def __getitem__(self, name):
        return self.bufs[name]

    def intact(self, after):
        torch.cuda.synchronize()
        for name, g in self.bufs.items():
            g.assert_intact("%s after %s" % (name, after))

    def snapshot(self):
        return {n: g.snapshot() for n, g in self.bufs.items()}

    def assert_unchanged(self, snap, after):
        torch.cuda.synchronize()
        for name, g in self.bufs.items():
            assert g.unchanged_since(snap[name]), "%s was written by %s" % (name, after)


def assert_same_bits(runs, what):
    """runs: {poison: {name: ndarray}}.  Every array has the same bytes under every poison."""
    ps = list(runs)
    for p in ps[1:]:
        assert runs[p].keys() == runs[ps[0]].keys()
        for name, a in runs[ps[0]].items():
            b = runs[p][name]
            same = a.shape == b.shape and a.tobytes() == b.tobytes()
            if not same:
                d = np.nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))[0]
                raise AssertionError("%s: %s depends on what the buffers held on entry: poison 0x%02X and 0x%02X differ in %d bytes "
                                     "(first at byte %d)" % (what, name, ps[0], p, d.size, int(d[0]) if d.size else -1))
