"""A guarded allocator for tests (test code only: the product allocates exactly as before).

The C interface's contract is that the caller owns all memory and a ``*_bytes`` query gives the size of a context / scratch buffer.  The
tests normally allocate through torch's caching allocator, which rounds to 512 B and hands out pieces of much larger blocks, so a store
past the end of a buffer lands in memory that belongs to the process and nothing notices.  Here every buffer is carved out of one uint8
allocation laid out as

    [ guard | payload | guard ]

with the payload at a 256-byte aligned address (what hipMalloc and torch give every caller), EXACTLY as long as asked for (the guard begins
at ``nbytes``, not at ``max(nbytes, at_least)``), and filled with a chosen byte: 0xFF (NaN as float32, -1 as int32: the project's existing
poison, so a value that is read before the library wrote it shows in the results) or 0x00.  The guards are filled with 0xA5 -- 0xFF
around a typed INPUT (``Guard.copy``), so that a row read past its end is NaN and poisons the result -- and ``Guard.check()`` asserts that
not one of their bytes changed.

Guard width: 64 KiB on either side.  The widest single tile store of the library is 32 rows x 256 columns x 4 B = 32 KiB (the layer
kernels' 32-row output tile at the widest accepted layer, cnr_gemm*.hip; the weight-gradient kernels store 256 x 256 tiles but row by row
into [n_out][k] tensors, at most 256 x 4 B = 1 KiB contiguous per row), so a one-tile overrun -- a last tile whose rows are not masked at
P, or columns not masked at n_out -- stays inside the allocation: it is reported, it does not fault.  No wider store was found when reading
the kernels for this module.

``Guard.scratch_substituted()`` replaces ``RenderLibrary.scratch`` -- the one place the package allocates context and scratch buffers -- for
the duration of a case and records, for every buffer, the size function's name, its arguments and the region."""
import contextlib
import ctypes as C

import torch

GUARD_BYTES = 64 << 10
GUARD_FILL = 0xA5
ALIGN = 256
POISON = 0xFF


class Region:
    """One guarded buffer: ``raw`` = [guard | payload | guard], the payload is raw[off : off + nbytes]."""

    def __init__(self, raw, off, nbytes, what, args, zero, around=GUARD_FILL):
        self.raw, self.off, self.nbytes, self.what, self.args, self.zero, self.around = raw, off, nbytes, what, args, zero, around

    @property
    def payload(self):
        return self.raw[self.off:self.off + self.nbytes]

    def changed(self):
        """None, or a description of the guard bytes that changed (offsets relative to the payload's END: >= 0 behind it, < -nbytes in front)."""
        end = self.off + self.nbytes
        msgs = []
        for name, lo, hi in (("before", 0, self.off), ("after", end, self.raw.numel())):
            bad = (self.raw[lo:hi] != self.around).nonzero().reshape(-1)
            if bad.numel():
                first, last = int(bad[0]) + lo - end, int(bad[-1]) + lo - end
                msgs.append("%d guard byte(s) %s the payload changed, offsets %+d .. %+d from the payload's end" % (bad.numel(), name, first, last))
        if self.zero and self.nbytes and bool((self.payload != 0).any()):
            nz = (self.payload != 0).nonzero().reshape(-1)
            msgs.append("zero-contract buffer left non-zero: %d byte(s), payload offsets %d .. %d" % (nz.numel(), int(nz[0]), int(nz[-1])))
        if not msgs:
            return None
        return "%s%r (%d bytes): %s" % (self.what, tuple(self.args), self.nbytes, "; ".join(msgs))


def _carve(nbytes, device, fill, around=GUARD_FILL):
    nbytes = int(nbytes)
    raw = torch.empty(GUARD_BYTES + ALIGN + nbytes + GUARD_BYTES, dtype=torch.uint8, device=device)
    off = GUARD_BYTES + (-(raw.data_ptr() + GUARD_BYTES)) % ALIGN
    raw.fill_(around)
    raw[off:off + nbytes].fill_(fill)
    assert (raw.data_ptr() + off) % ALIGN == 0 and off >= GUARD_BYTES and raw.numel() - off - nbytes >= GUARD_BYTES
    return raw, off


def guarded(nbytes, device, fill=POISON, what="bytes", args=(), zero=False, around=GUARD_FILL):
    """Region of ``nbytes`` payload bytes on ``device`` filled with ``fill`` (its ``.payload`` is the uint8 tensor to hand out).  ``around``:
    the guards' byte -- 0xA5 by default; 0xFF around an INPUT, so that a row read past its end is NaN and poisons the result."""
    raw, off = _carve(nbytes, device, fill, around)
    return Region(raw, off, int(nbytes), what, args, zero, around)


def guarded_empty(shape, dtype, device, fill=POISON, what="tensor", around=GUARD_FILL):
    """(tensor of ``shape`` / ``dtype`` whose storage is a guarded payload, its Region); see ``guarded`` for ``around``."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    n = 1
    for s in shape:
        n *= s
    reg = guarded(n * torch.empty(0, dtype=dtype).element_size(), device, fill, what, (shape, str(dtype).replace("torch.", "")), around=around)
    return reg.payload.view(dtype).reshape(shape), reg


def _plain(a):
    """A recorded argument in printable form: ctypes structures behind byref() as {field: value}, arrays as lists."""
    a = getattr(a, "_obj", a)
    if isinstance(a, C.Structure):
        return {f[0]: getattr(a, f[0]) for f in a._fields_}
    if isinstance(a, C.Array):
        return list(a)
    return a


class Guard:
    """The guarded buffers of one case.  ``fill``: the payload byte of buffers whose contents need not be initialised (0xFF or 0x00);
    a buffer asked for with ``zero=True`` (a documented zero contract) always starts as 0x00 and must be all zero again at check()."""

    def __init__(self, fill=POISON):
        self.fill = fill
        self.regions = []
        self._typed = []        # (tensor, region) of empty() / copy()
        self.names = set()      # size functions seen by the substituted RenderLibrary.scratch

    def bytes(self, nbytes, device, what="bytes", args=(), zero=False):
        reg = guarded(nbytes, device, 0x00 if zero else self.fill, what, args, zero)
        self.regions.append(reg)
        return reg.payload

    def empty(self, shape, dtype, device, what="tensor", fill=None, around=GUARD_FILL):
        t, reg = guarded_empty(shape, dtype, device, self.fill if fill is None else fill, what, around)
        self.regions.append(reg)
        self._typed.append((t, reg))
        return t

    def addr(self, t):
        """The address of a tensor made by empty() / copy() as a pointer argument -- also of a zero-length one, which has no data_ptr()
        of its own but still a place between its guards."""
        for u, reg in self._typed:
            if u is t:
                return C.c_void_p(reg.raw.data_ptr() + reg.off)
        raise KeyError("not a tensor of this guard")

    def copy(self, t, what="input"):
        """``t`` copied into a guarded tensor of the same shape and dtype with 0xFF (NaN) on either side: an input the library may
        neither read past (the NaN would show in the results) nor write around."""
        t = t.detach().contiguous()
        g = self.empty(t.shape, t.dtype, t.device, what, around=POISON)
        g.copy_(t)
        return g

    @contextlib.contextmanager
    def scratch_substituted(self):
        """RenderLibrary.scratch allocates from this guard: payload of exactly the bytes the size function said."""
        from color_neus_amd import _lib
        guard, orig = self, _lib.RenderLibrary.scratch

        def scratch(lib, bytes_fn, device, *args, at_least=0, zero=False, nbytes=None):
            if nbytes is None:      # a size function: recorded by name; a stated size: by the entry point's name and the byte count
                nb = getattr(lib.lib, bytes_fn)(*args)
                guard.names.add(bytes_fn)
                rec = tuple(_plain(a) for a in args)
            else:
                nb, rec = int(nbytes), ("nbytes=%d" % int(nbytes),)
            return guard.bytes(nb, device, bytes_fn, rec, zero), nb

        _lib.RenderLibrary.scratch = scratch
        try:
            yield self
        finally:
            _lib.RenderLibrary.scratch = orig

    def check(self):
        """Synchronise, then assert that every guard byte before and after every payload is unchanged (and zero-contract payloads are
        zero); the message names the size function, its arguments and the first / last offset and count of the changed bytes."""
        if any(r.raw.is_cuda for r in self.regions):
            torch.cuda.synchronize()
        bad = [m for m in (r.changed() for r in self.regions) if m is not None]
        assert not bad, "\n".join(bad)
