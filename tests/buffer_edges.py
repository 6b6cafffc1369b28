"""Hostile surroundings for the buffers handed to the device entry points (tests/test_buffer_edges_*.py).

The contract ("Buffer edges"): the strictly-upper elements of the square diagonal
blocks are ignored on input, operands declared read-only are not written, vector blocks are touched on
their first `order` rows of every column only, and nothing outside the operands is written.  Here:

  SENTINEL / SENTINEL_BITS  a quiet NaN with a fixed payload per dtype, compared as integer words
  upper_words(sol)          the indices of the strictly-upper diagonal-block elements
  poison_upper(t, sol)      the sentinel into those elements (host array or device tensor)
  Frame                     one buffer full of the sentinel that holds several payloads, each between
                            guards and at an odd element offset (element-aligned, not 16-byte-aligned)
  strided / unpack / assert_padding_intact
                            right-hand sides with leading dimension ld > n and sentinel padding rows

Nothing here touches the GPU at import; Frame allocates on the device it is given."""
import numpy as np

from autograd_ref import element_coords
from known_factor import bitwise_equal

SENTINEL_BITS = {np.dtype(np.float64): 0x7FF80000DEADBEEF, np.dtype(np.float32): 0x7FC0BEEF}
_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}
SENTINEL = {dt: np.array([bits], dtype=_UINT[dt]).view(dt)[0] for dt, bits in SENTINEL_BITS.items()}
for _dt in list(SENTINEL):
    SENTINEL[_dt.type] = SENTINEL[_dt]
    SENTINEL_BITS[_dt.type] = SENTINEL_BITS[_dt]
GUARD = 4096


def _words(a):
    """host array as unsigned integer words"""
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype])


def _bits(t):
    """device / host torch tensor as signed integer words (the sentinels are positive in both widths)"""
    import torch
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _np_dtype(t):
    import torch
    return np.dtype(np.float64 if t.dtype == torch.float64 else np.float32)


def is_sentinel(a):
    """boolean array: which words of the host array hold the sentinel bits"""
    return _words(a) == _UINT[a.dtype](SENTINEL_BITS[a.dtype])


def upper_words(sol):
    """indices into the numeric data of the strictly-upper elements of the square diagonal blocks:
    ~lowerMask(), asserted against the i < j of autograd_ref.element_coords (cached on the solver)"""
    got = getattr(sol, "_buffer_edges_upper", None)
    if got is None:
        got = np.nonzero(~sol.lowerMask())[0].astype(np.int64)
        i, j = element_coords(sol)
        assert np.array_equal(got, np.nonzero(i < j)[0]), "lowerMask() and element_coords disagree"
        sol._buffer_edges_upper = got
    return got


def poison_upper(t, sol):
    """the sentinel into every strictly-upper diagonal-block element of `t` (the solver's layout; a host
    array or a device tensor, changed in place and returned)"""
    idx = upper_words(sol)
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"] and t.size == sol.dataSize()
        t.view(_UINT[t.dtype])[idx] = SENTINEL_BITS[t.dtype]
        return t
    import torch
    assert t.numel() == sol.dataSize() and t.is_contiguous()
    if len(idx):
        _bits(t)[torch.from_numpy(idx).to(t.device)] = SENTINEL_BITS[_np_dtype(t)]
    return t


def clear_upper(a, sol, value=0.0):
    """host copy of `a` with `value` in the strictly-upper diagonal-block elements (the plain,
    unpoisoned twin of a poisoned operand)"""
    out = np.array(a, copy=True)
    out[upper_words(sol)] = value
    return out


class Frame:
    """One 1-D tensor full of the sentinel that holds the payloads of the given sizes.  Every payload has
    at least `guard` sentinel words on both sides and starts at an odd element offset from the base (the
    first guard is one word longer, and so is any later guard that would end on an even offset): a
    payload is element-aligned and never 16-byte-aligned when the base is.  With align_bytes (a multiple of
    the element size; 16 for the work areas of the iterative pieces) every payload instead starts at a
    multiple of align_bytes from address zero, still behind at least `guard` sentinel words; a payload of
    exactly the documented size then has its first foreign word right behind its last own one.

    view(k)        the contiguous slice of payload k (what the library is handed)
    fill(k, a)     host array -> payload k, word for word
    host(k)        payload k as a host array
    seal()         remembers the payloads as they are now
    assert_intact  every word outside the payloads still holds the sentinel, and the payloads named
                   read_only are bitwise what they were at seal()"""

    def __init__(self, sizes, dtype, guard=GUARD, device="cuda", align_bytes=None):
        import torch
        self.dtype = np.dtype(dtype)
        self.guard = int(guard)
        self.sizes = [int(s) for s in sizes]
        self.align_bytes = None if align_bytes is None else int(align_bytes)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        if self.align_bytes is not None:
            self._init_aligned(torch, tdt, device)
            return
        self.offsets = []
        at = 0
        for s in self.sizes:
            at += self.guard
            at += 1 - at % 2
            self.offsets.append(at)
            at += s
        self.total = at + self.guard
        self.base = torch.empty(self.total, dtype=tdt, device=device)
        _bits(self.base).fill_(SENTINEL_BITS[self.dtype])
        if self.base.is_cuda:
            assert self.base.data_ptr() % 512 == 0, "the allocator's alignment is not what the frame assumes"
        assert all(o % 2 == 1 for o in self.offsets) and self.offsets[0] == self.guard + 1
        self._sealed = None

    def _init_aligned(self, torch, tdt, device):
        """the layout of align_bytes: the offsets are taken from the address the allocator returned"""
        item = self.dtype.itemsize
        assert self.align_bytes > 0 and self.align_bytes % item == 0, (self.align_bytes, item)
        step = self.align_bytes // item
        self.total = sum(self.sizes) + (len(self.sizes) + 1) * self.guard + (len(self.sizes) + 1) * step
        self.base = torch.empty(self.total, dtype=tdt, device=device)
        _bits(self.base).fill_(SENTINEL_BITS[self.dtype])
        assert self.base.data_ptr() % item == 0
        first = self.base.data_ptr() // item          # the base's address in elements
        self.offsets = []
        at = 0
        for s in self.sizes:
            at += self.guard
            at += -(first + at) % step
            self.offsets.append(at)
            at += s
        assert at + self.guard <= self.total
        assert all((self.base.data_ptr() + o * item) % self.align_bytes == 0 for o in self.offsets)
        self._sealed = None

    def __len__(self):
        return len(self.sizes)

    def view(self, k):
        o = self.offsets[k]
        return self.base[o:o + self.sizes[k]]

    def views(self):
        return [self.view(k) for k in range(len(self.sizes))]

    def fill(self, k, a):
        import torch
        a = np.ascontiguousarray(a).ravel()
        assert a.dtype == self.dtype and a.size == self.sizes[k], (a.dtype, a.size, self.sizes[k])
        words = torch.from_numpy(a.view(np.int64 if self.dtype == np.float64 else np.int32).copy())
        _bits(self.view(k)).copy_(words)
        return self

    def host(self, k):
        return self.view(k).cpu().numpy().copy()

    def seal(self):
        self._sealed = self.base.clone()
        return self

    def _gaps(self):
        at = 0
        for o, s in zip(self.offsets, self.sizes):
            yield at, o
            at = o + s
        yield at, self.total

    def assert_intact(self, read_only=(), what=""):
        import torch
        bits = _bits(self.base)
        for k, (a, b) in enumerate(self._gaps()):
            bad = bits[a:b] != SENTINEL_BITS[self.dtype]
            if bool(bad.any()):
                at = a + int(torch.nonzero(bad)[0, 0])
                near = [q for q in range(len(self.sizes))
                        if at == self.offsets[q] - 1 or at == self.offsets[q] + self.sizes[q]]
                raise AssertionError(("a word outside the payloads was written", what, "word %d" % at,
                                      "%d words changed in the guard before payload %d" % (int(bad.sum()), k),
                                      "next to payload %s" % near if near else "inside the guard"))
        if read_only:
            assert self._sealed is not None, "assert_intact(read_only=...) needs seal() first"
            was = _bits(self._sealed)
            for k in read_only:
                o, s = self.offsets[k], self.sizes[k]
                if not torch.equal(bits[o:o + s], was[o:o + s]):
                    n = int((bits[o:o + s] != was[o:o + s]).sum())
                    raise AssertionError(("a read-only operand was written", what, "payload %d" % k, "%d words" % n))


def framed(dtype, arrays, device="cuda", guard=GUARD):
    """a sealed Frame whose payloads hold the given host arrays"""
    fr = Frame([np.asarray(a).size for a in arrays], dtype, guard=guard, device=device)
    for k, a in enumerate(arrays):
        fr.fill(k, np.asarray(a, dtype=fr.dtype))
    return fr.seal()


# ---- right-hand sides with a leading dimension ---------------------------------------------------

def strided(b, ld, dtype):
    """the n x nRHS right-hand sides `b` as nRHS columns of stride ld >= n (host array of nRHS * ld
    elements in `dtype`), the padding rows holding the sentinel"""
    b = np.asarray(b)
    b = b.reshape(b.shape[0], -1)
    n, nrhs = b.shape
    assert ld >= n
    dt = np.dtype(dtype)
    out = np.empty((nrhs, ld), dtype=dt)
    out.view(_UINT[dt])[:] = SENTINEL_BITS[dt]
    out[:, :n] = b.T.astype(dt)
    return out.ravel()


def unpack(v, n, ld, nrhs):
    """inverse of strided: the n x nRHS block of the packed vector, in float64"""
    v = np.asarray(v)
    assert v.size == nrhs * ld
    return v.reshape(nrhs, ld)[:, :n].T.astype(np.float64)


def assert_padding_intact(v, n, ld, nrhs, what=""):
    """the rows n .. ld of every column of the packed host vector still hold the sentinel"""
    v = np.ascontiguousarray(v)
    assert v.size == nrhs * ld
    pad = is_sentinel(v).reshape(nrhs, ld)[:, n:]
    if not pad.all():
        col, row = np.argwhere(~pad)[0]
        raise AssertionError(("a padding row was written", what, "row %d of column %d" % (n + row, col),
                              "%d words" % int((~pad).sum())))


__all__ = ["SENTINEL", "SENTINEL_BITS", "GUARD", "Frame", "framed", "upper_words", "poison_upper", "clear_upper",
           "is_sentinel", "strided", "unpack", "assert_padding_intact", "bitwise_equal"]
