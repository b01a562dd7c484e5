"""Guard-band tensors for the memory-safety tests (tests/test_hip_bounds.py, tests/test_hip_net_memory.py).

A guarded tensor is an ordinary contiguous tensor that is a view into a larger uint8 buffer: a band of known bytes lies in front of its
first element and another starts at the first byte past its last element.  A kernel that stores outside the tensor changes a band, and
check_bands() says which one and where.  A kernel that never stores an element leaves the tensor's prefill (0xff bytes: NaN in fp16, fp32
and fp64) where a value should be.

What this cannot see: a stray access FURTHER OUT than the band (each band is max(64 KiB, one innermost row of the tensor)), and a stray
READ whose value never reaches a result (a band cannot tell that it was read)."""
import itertools

import torch

BAND_BYTES = 64 << 10
FILLS = ("ff", "zero", "random")
_seeds = itertools.count(1)


class _Guard:
    __slots__ = ("buf", "front", "nbytes", "band", "saved_front", "saved_rear", "name")


def _random_bytes(n, seed):
    return torch.randint(0, 256, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _pattern(kind, n, seed):
    if kind == "ff":
        return torch.full((n,), 255, dtype=torch.uint8)
    if kind == "zero":
        return torch.zeros(n, dtype=torch.uint8)
    if kind == "random":
        return _random_bytes(n, seed)
    raise ValueError("fill / bands must be one of %r, got %r" % (FILLS, kind))


def guarded_empty(shape, dtype, device="cpu", fill="ff", bands="random", name=None, align=16):
    """A contiguous `dtype` tensor of `shape` on `device` between two bands.

    fill : the tensor's own bytes: "ff" (every byte 0xff: NaN as fp16 / fp32 / fp64, 255 as uint8, -1 as a signed integer), "zero", or
           "random" (seeded bytes).
    bands: "random" (default: seeded bytes, different for every tensor, so that a stray store of zeros or of any one constant shows) or
           "ff" (for INPUTS of float kernels: what an over-read fetches decodes as NaN and poisons the result it reaches).
    The first element is `align`-byte aligned (the kernels need 16); the rear band starts at the first byte past the last element, whatever
    nbytes % 16 is.  Each band is at least 64 KiB and at least one innermost-stride row of the tensor (shape[-1] elements): a stray access
    further out than that is NOT detected."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    esz = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= s
    nbytes = numel * esz
    row = (shape[-1] if shape else 1) * esz
    band = -(-max(BAND_BYTES, row) // align) * align
    buf = torch.empty(band + align + nbytes + band, dtype=torch.uint8, device=device)
    front = band + (-(buf.data_ptr() + band)) % align           # >= band bytes in front, and the tensor starts on an `align` boundary
    seed = next(_seeds)
    g = _Guard()
    g.buf, g.front, g.nbytes, g.band = buf, front, nbytes, band
    g.name = name or "%s%s" % (str(dtype).replace("torch.", ""), list(shape))
    rear = buf.numel() - front - nbytes                          # >= band
    buf[:front] = _pattern(bands, front, 2 * seed).to(device)
    buf[front + nbytes:] = _pattern(bands, rear, 2 * seed + 1).to(device)
    if nbytes:
        buf[front:front + nbytes] = _pattern(fill, nbytes, 7919 * seed).to(device)
    g.saved_front, g.saved_rear = buf[:front].clone(), buf[front + nbytes:].clone()
    t = buf[front:front + nbytes].view(dtype).view(shape)
    assert t.is_contiguous() and (nbytes == 0 or (t.data_ptr() % align == 0 and t.data_ptr() == buf.data_ptr() + front))
    t._guard = g
    return t


def guarded_like(t, fill="ff", bands="random", name=None, device=None, align=16):
    """guarded_empty of t's shape and dtype (on `device`, else t's)"""
    return guarded_empty(t.shape, t.dtype, device if device is not None else t.device, fill, bands, name, align)


def guarded_copy(t, device=None, name=None, bands="ff"):
    """an INPUT: t's values in a guarded tensor (on `device`, else t's) whose bands are 0xff bytes, i.e. NaN to a float kernel that reads past an end"""
    g = guarded_like(t, "zero", bands, name, device)
    g.copy_(t)
    return g


def refill(t, fill):
    """overwrite the tensor's own bytes with a fill pattern again (the bands stay)"""
    g = t._guard
    if g.nbytes:
        g.buf[g.front:g.front + g.nbytes] = _pattern(fill, g.nbytes, 7919 * next(_seeds)).to(g.buf.device)
    return t


def raw_bytes(t):
    """the tensor's own bytes as a uint8 view"""
    g = t._guard
    return g.buf[g.front:g.front + g.nbytes]


def backing(t):
    """(the uint8 buffer the tensor lives in, byte offset of its first element): for tests of the harness itself"""
    return t._guard.buf, t._guard.front


def check_bands(*tensors):
    """every band of every guarded tensor still equals its saved copy bit for bit; else AssertionError naming the tensor, the band, and the
    first differing byte (offset inside the band, and relative to the tensor: negative in front of element 0, from 0 up past the last byte)"""
    for t in tensors:
        g = getattr(t, "_guard", None)
        assert g is not None, "check_bands: not a guarded tensor (views of one lose the guard: pass the tensor guarded_* returned)"
        for which, now, saved in (("front", g.buf[:g.front], g.saved_front), ("rear", g.buf[g.front + g.nbytes:], g.saved_rear)):
            if torch.equal(now, saved):
                continue
            bad = (now != saved).nonzero()
            off = int(bad[0])
            rel = off - g.front if which == "front" else off
            raise AssertionError("%s: %s band changed at byte %d of the band (%s; %d bytes differ, was 0x%02x, is 0x%02x)"
                                 % (g.name, which, off, "%d bytes before the first element" % -rel if which == "front" else
                                    "%d bytes past the last element" % rel, bad.numel(), int(saved[off]), int(now[off])))
