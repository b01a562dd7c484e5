"""The guard-band harness (tests/guarded.py) bites: on the CPU, a one-byte write into either band is reported with its offset, the
tensor sits aligned and flush against its rear band for every dtype and odd size, and the fills are what they claim."""
import math

import pytest
import torch

from guarded import BAND_BYTES, backing, check_bands, guarded_copy, guarded_empty, guarded_like, raw_bytes, refill

DTYPES = [torch.uint8, torch.float16, torch.int32, torch.float32, torch.float64]
SHAPES = [(1,), (3,), (7, 5), (37, 53, 3), (2, 5, 7, 12), ()]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_alignment_and_flushness(dtype, shape):
    t = guarded_empty(shape, dtype)
    buf, front = backing(t)
    assert t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
    assert t.data_ptr() % 16 == 0
    assert t.data_ptr() == buf.data_ptr() + front
    nbytes = t.numel() * t.element_size()
    assert front >= BAND_BYTES and buf.numel() - front - nbytes >= BAND_BYTES
    # flush: the byte right after the last element is the rear band's first byte, also where nbytes % 16 != 0
    for where in (front - 1, front + nbytes):
        old = int(buf[where])
        buf[where] = old ^ 0x01
        with pytest.raises(AssertionError):
            check_bands(t)
        buf[where] = old
        check_bands(t)
    # ... and the first and last byte of the tensor itself belong to no band
    if nbytes:
        raw_bytes(t)[0] ^= 0x55
        raw_bytes(t)[-1] ^= 0x55
        check_bands(t)


def test_alignment_on_request_and_wide_rows():
    t = guarded_empty((3, 5), torch.uint8, align=256)
    assert t.data_ptr() % 256 == 0
    wide = guarded_empty((2, 3 * BAND_BYTES // 4 + 1), torch.float32)     # one row is more than 64 KiB: the band grows to hold it
    buf, front = backing(wide)
    row = wide.shape[1] * 4
    assert front >= row and buf.numel() - front - wide.numel() * 4 >= row
    check_bands(t, wide)


@pytest.mark.parametrize("offset", [0, 1, 4097, BAND_BYTES - 1])
def test_one_byte_write_into_either_band_is_reported_with_its_offset(offset):
    t = guarded_empty((5, 3), torch.float16, name="victim")          # 30 bytes: nbytes % 16 != 0
    buf, front = backing(t)
    check_bands(t)
    # rear band: `offset` bytes past the last element
    where = front + 30 + offset
    old = int(buf[where])
    buf[where] = (old + 1) % 256
    with pytest.raises(AssertionError, match=r"victim: rear band changed at byte %d of the band \(%d bytes past the last element" % (offset, offset)):
        check_bands(t)
    buf[where] = old
    check_bands(t)
    # front band: `offset + 1` bytes before the first element
    where = front - 1 - offset
    old = int(buf[where])
    buf[where] = (old + 1) % 256
    with pytest.raises(AssertionError, match=r"victim: front band changed at byte %d of the band \(%d bytes before the first element" % (where, offset + 1)):
        check_bands(t)
    buf[where] = old
    check_bands(t)


def test_a_stray_store_of_zeros_or_of_one_constant_is_seen():
    """band bytes are seeded random bytes, not a constant: whichever constant a stray 16-byte store writes, it changes the band"""
    for value in (0, 255, 0x3c):
        t = guarded_empty((9,), torch.float32)
        buf, front = backing(t)
        buf[front + 36:front + 52] = value
        with pytest.raises(AssertionError, match="rear band changed at byte"):
            check_bands(t)
    a, b = guarded_empty((4,), torch.uint8), guarded_empty((4,), torch.uint8)
    assert not torch.equal(backing(a)[0][:64], backing(b)[0][:64])          # another seed per tensor


def test_fills():
    for dtype in (torch.float16, torch.float32, torch.float64):
        assert bool(torch.isnan(guarded_empty((7, 3), dtype, fill="ff")).all())
    assert bool((guarded_empty((7, 3), torch.uint8, fill="ff") == 255).all())
    assert bool((guarded_empty((7,), torch.int32, fill="ff") == -1).all())
    for dtype in DTYPES:
        z = guarded_empty((7, 3), dtype, fill="zero")
        assert bool((z == 0).all()) and bool((raw_bytes(z) == 0).all())
    r = raw_bytes(guarded_empty((4096,), torch.float32, fill="random"))
    hist = torch.bincount(r.long(), minlength=256)
    assert int((hist > 0).sum()) == 256 and int(hist.max()) < 4 * 16384 // 256      # every byte value, none dominating
    with pytest.raises(ValueError):
        guarded_empty((3,), torch.float32, fill="ones")


def test_input_copies_have_nan_bands_and_refill_keeps_the_bands():
    x = torch.arange(35, dtype=torch.float32).view(5, 7)
    g = guarded_copy(x)
    assert torch.equal(g, x)
    buf, front = backing(g)
    assert bool((buf[:front] == 255).all()) and bool((buf[front + 140:] == 255).all())
    assert math.isnan(float(buf[front + 140:front + 144].view(torch.float32)))          # what a one-element over-read fetches
    like = guarded_like(x, "zero")
    assert like.shape == x.shape and like.dtype == x.dtype and float(like.abs().sum()) == 0.0
    refill(like, "ff")
    assert bool(torch.isnan(like).all())
    check_bands(g, like)


def test_check_bands_refuses_what_it_cannot_check():
    t = guarded_empty((4, 4), torch.float32)
    with pytest.raises(AssertionError, match="not a guarded tensor"):
        check_bands(t[1:])
    with pytest.raises(AssertionError, match="not a guarded tensor"):
        check_bands(torch.zeros(3))
