"""YCbCr <-> RGB on the device (cfen_yuv_to_rgb_u8, cfen_rgb_to_yuv_u8; ops.yuv_to_rgb_u8, ops.rgb_to_yuv_u8) against the numpy restatement
tests/yuv_ref.py.  Everything is integer arithmetic, so every comparison is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, yuv
import guarded
import yuv_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (H, W).  3 x 5 and 17 x 33 have an odd number of luma bytes: their chroma planes start at odd addresses.  130 x 259: rows of odd length, so
# image rows and the rows of both planes change their alignment from one to the next; more than one block per frame both ways
SIZES = [(1, 1), (2, 2), (3, 5), (17, 33), (64, 64), (130, 259)]
TABLES = [("bt601", False), ("bt709", True)]
_CACHE = {}


def case(H, W, chroma, matrix, full):
    """(frames (2, nbytes) uint8 random bytes -- out-of-gamut YCbCr included --, their RGB, rgb (2,H,W,3) random, its frames): computed once"""
    key = (H, W, chroma, matrix, full)
    if key not in _CACHE:
        rs = np.random.RandomState(hash((H, W, len(chroma))) % 2 ** 31)
        n = ref.frame_bytes(H, W, chroma)
        frames = rs.randint(0, 256, (2, n)).astype(np.uint8)
        frames[1, :min(n, 8)] = (0, 255, 0, 255, 16, 235, 240, 1)[:min(n, 8)]
        rgb = rs.randint(0, 256, (2, H, W, 3)).astype(np.uint8)
        want_rgb = np.stack([ref.yuv_to_rgb(f, H, W, chroma, matrix, full) for f in frames])
        want_frames = np.stack([ref.rgb_to_yuv(x, chroma, matrix, full) for x in rgb])
        for a in (frames, rgb, want_rgb, want_frames):
            a.setflags(write=False)
        _CACHE[key] = (frames, want_rgb, rgb, want_frames)
    return _CACHE[key]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def test_frame_bytes_and_the_offsets_the_cases_claim():
    q = _lib.load().cfen_yuv_frame_bytes
    for H, W in SIZES + [(65536, 65536), (1, 65536)]:
        for chroma, code in yuv.CHROMA.items():
            assert q(H, W, code) == ref.frame_bytes(H, W, chroma) == yuv.frame_bytes(H, W, chroma)
    assert q(0, 4, 0) == 0 and q(4, 0, 0) == 0 and q(65537, 4, 0) == 0 and q(4, 65537, 0) == 0 and q(4, 4, 5) == 0 and q(4, 4, -1) == 0
    assert (17 * 33) % 2 == 1                                          # odd W and H: the chroma planes of 17 x 33 start at odd addresses
    assert (3 * 5) % 2 == 1 and ref.chroma_shape(3, 5, "420jpeg") == (2, 3)


@pytest.mark.parametrize("matrix,full", TABLES)
@pytest.mark.parametrize("chroma", ref.CHROMAS)
@pytest.mark.parametrize("H,W", SIZES)
def test_both_directions_equal_the_restatement(H, W, chroma, matrix, full):
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, matrix, full)
    got = ops.yuv_to_rgb_u8(dev(frames), H, W, chroma, matrix, full)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, H, W, 3)
    bad = int((got.cpu().numpy() != want_rgb).sum())
    print("to rgb: %d of %d bytes differ" % (bad, want_rgb.size))
    assert bad == 0
    back = ops.rgb_to_yuv_u8(dev(rgb), chroma, matrix, full)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (2, ref.frame_bytes(H, W, chroma))
    bad = int((back.cpu().numpy() != want_frames).sum())
    print("to yuv: %d of %d bytes differ%s" % (bad, want_frames.size, " (first at %s)" % (np.argwhere(back.cpu().numpy() != want_frames)[:4].tolist(),) if bad else ""))
    assert bad == 0
    if (H, W) == (130, 259):                                            # the clamps are hit, both ways
        assert (want_rgb == 0).any() and (want_rgb == 255).any()


@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_batch_stream_offset_and_stride_do_not_change_a_bit(chroma):
    H, W, matrix, full = 17, 33, "bt601", False
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, matrix, full)
    n = frames.shape[1]
    f3 = dev(np.concatenate([frames, frames[:1]]))
    x3 = dev(np.concatenate([rgb, rgb[:1]]))
    got3 = ops.yuv_to_rgb_u8(f3, H, W, chroma, matrix, full)
    back3 = ops.rgb_to_yuv_u8(x3, chroma, matrix, full)
    assert np.array_equal(got3.cpu().numpy(), np.concatenate([want_rgb, want_rgb[:1]]))
    assert np.array_equal(back3.cpu().numpy(), np.concatenate([want_frames, want_frames[:1]]))
    one = ops.yuv_to_rgb_u8(f3[1].clone(), H, W, chroma, matrix, full)                     # a frame alone (1-D in, (H,W,3) out)
    assert tuple(one.shape) == (H, W, 3) and torch.equal(one, got3[1])
    one = ops.rgb_to_yuv_u8(x3[1].clone(), chroma, matrix, full)
    assert tuple(one.shape) == (n,) and torch.equal(one, back3[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a, b = ops.yuv_to_rgb_u8(f3, H, W, chroma, matrix, full), ops.rgb_to_yuv_u8(x3, chroma, matrix, full)
    side.synchronize()
    assert torch.equal(a, got3) and torch.equal(b, back3)
    # both buffers at byte offsets 1 .. 3 of a larger one, frames frame_bytes + 5 apart
    stride, npx = n + 5, 3 * H * W * 3
    for off in (1, 2, 3):
        fb = torch.full((3 * stride + 8,), 0xAA, dtype=torch.uint8, device=DEV)
        fv = fb[off:off + 3 * stride].view(3, stride)[:, :n]
        fv.copy_(f3)
        xb = torch.zeros(npx + 8, dtype=torch.uint8, device=DEV)
        xv = xb[off:off + npx].view(3, H, W, 3)
        xv.copy_(x3)
        assert fv.data_ptr() % 4 == off and xv.data_ptr() % 4 == off and fv.stride(0) == stride
        ob = torch.zeros(npx + 8, dtype=torch.uint8, device=DEV)
        got = ops.yuv_to_rgb_u8(fv, H, W, chroma, matrix, full, out=ob[off:off + npx].view(3, H, W, 3))
        assert torch.equal(got, got3), off
        assert torch.equal(ops.yuv_to_rgb_u8(fv, H, W, chroma, matrix, full), got3), off        # aligned output, misaligned frames
        yb = torch.full((3 * stride + 8,), 0x55, dtype=torch.uint8, device=DEV)
        yv = yb[off:off + 3 * stride].view(3, stride)[:, :n]
        ops.rgb_to_yuv_u8(xv, chroma, matrix, full, out=yv)
        assert torch.equal(yv, back3), off
        gaps = yb[off:off + 3 * stride].view(3, stride)[:, n:]
        assert bool((gaps == 0x55).all()) and bool((yb[:off] == 0x55).all()) and bool((yb[off + 3 * stride:] == 0x55).all())
        assert torch.equal(ops.rgb_to_yuv_u8(x3, chroma, matrix, full, out=yv), back3), off     # aligned images, misaligned frames


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------
def test_guard_bands_yuv():
    """inputs between 0xff bands, outputs prefilled 0xff, zeros and random bytes between random bands: no band changes, every payload byte is
    written (the result is the unguarded call's whatever the prefill), the gap between two frames keeps its bytes"""
    lib = _lib.load()
    for (H, W), chroma in (((17, 33), "420jpeg"), ((130, 259), "420mpeg2"), ((3, 5), "422"), ((17, 33), "444"), ((2, 2), "mono"), ((1, 1), "420jpeg")):
        matrix, full = "bt709", True
        code = yuv.CHROMA[chroma]
        frames, want_rgb, rgb, want_frames = case(H, W, chroma, matrix, full)
        n = lib.cfen_yuv_frame_bytes(H, W, code)
        assert n == frames.shape[1]
        stride = n + 5
        fwd, inv, oy = yuv.tables(matrix, full)
        strided = np.zeros((2, stride), dtype=np.uint8)
        strided[:, :n] = frames
        gin = guarded.guarded_copy(dev(strided))
        gout = guarded.guarded_empty((2, H, W, 3), torch.uint8, DEV)
        for fill in guarded.FILLS:
            guarded.refill(gout, fill)
            _lib.check(lib.cfen_yuv_to_rgb_u8(_lib.ptr(gin), stride, 2, H, W, code, ops.yuv_table(inv, oy), _lib.ptr(gout), _lib.current_stream()), "yuv_to_rgb_u8")
            torch.cuda.synchronize()
            guarded.check_bands(gin, gout)
            assert np.array_equal(gout.cpu().numpy(), want_rgb), (H, W, chroma, fill)
        gin = guarded.guarded_copy(dev(rgb))
        gout = guarded.guarded_empty((2, stride), torch.uint8, DEV)
        for fill in guarded.FILLS:
            guarded.refill(gout, fill)
            before = gout.clone()
            _lib.check(lib.cfen_rgb_to_yuv_u8(_lib.ptr(gin), 2, H, W, code, ops.yuv_table(fwd, oy), _lib.ptr(gout), stride, _lib.current_stream()), "rgb_to_yuv_u8")
            torch.cuda.synchronize()
            guarded.check_bands(gin, gout)
            assert np.array_equal(gout[:, :n].cpu().numpy(), want_frames), (H, W, chroma, fill)
            assert torch.equal(gout[:, n:], before[:, n:]), (H, W, chroma, fill)                 # the stride gap
        assert lib.cfen_yuv_frame_bytes(H, W, code) == ref.frame_bytes(H, W, chroma)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    lib = _lib.load()
    H, W, chroma = 3, 5, "420jpeg"
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, "bt601", False)
    n = frames.shape[1]
    fwd, inv, oy = yuv.tables("bt601", False)
    f, x = dev(frames), dev(rgb)
    out_rgb = torch.full((2, H, W, 3), 7, dtype=torch.uint8, device=DEV)
    out_f = torch.full((2, n), 7, dtype=torch.uint8, device=DEV)
    z = ctypes.c_void_p(0)

    def table(t, oy_=oy, reserved=None, coef=None):
        c = ops.yuv_table(t, oy_)
        if reserved is not None:
            c.reserved[reserved] = 1
        if coef is not None:
            c.coef[4] = coef
        return c
    good = dict(frames=_lib.ptr(f), stride=n, B=2, H=H, W=W, chroma=0, table=table(inv), rgb=_lib.ptr(out_rgb))
    bad = [("frames", z, b"null pointer"), ("rgb", z, b"null pointer"), ("B", 0, b"B = 0"), ("B", 65536, b"B = 65536"), ("H", 0, b"H = 0"),
           ("W", 65537, b"W = 65537"), ("H", -3, b"H = -3"), ("chroma", 5, b"unknown chroma = 5"), ("chroma", -1, b"unknown chroma = -1"),
           ("stride", n - 1, b"frame_stride"), ("table", table(inv, reserved=0), b"reserved"), ("table", table(inv, reserved=5), b"reserved"),
           ("table", table(inv, oy_=256), b"luma_offset"), ("table", table(inv, coef=1 << 20), b"coefficients")]
    to_rgb = ("frames", "stride", "B", "H", "W", "chroma", "table", "rgb")
    to_yuv = ("rgb", "B", "H", "W", "chroma", "table", "frames", "stride")
    good2 = dict(good, frames=_lib.ptr(out_f), rgb=_lib.ptr(x), table=table(fwd))
    for key, value, what in bad:
        rc = lib.cfen_yuv_to_rgb_u8(*[dict(good, **{key: value})[k] for k in to_rgb], _lib.current_stream())
        err = lib.cfen_last_error()
        assert rc == -1 and b"yuv_to_rgb_u8" in err and what in err, (key, rc, err)
        rc = lib.cfen_rgb_to_yuv_u8(*[dict(good2, **{key: value})[k] for k in to_yuv], _lib.current_stream())
        err = lib.cfen_last_error()
        assert rc == -1 and b"rgb_to_yuv_u8" in err and what in err, (key, rc, err)
    torch.cuda.synchronize()
    assert bool((out_rgb == 7).all()) and bool((out_f == 7).all())
    _lib.check(lib.cfen_yuv_to_rgb_u8(*[good[k] for k in to_rgb], _lib.current_stream()), "yuv_to_rgb_u8")
    _lib.check(lib.cfen_rgb_to_yuv_u8(*[good2[k] for k in to_yuv], _lib.current_stream()), "rgb_to_yuv_u8")
    torch.cuda.synchronize()
    assert np.array_equal(out_rgb.cpu().numpy(), want_rgb) and np.array_equal(out_f.cpu().numpy(), want_frames)


def test_python_side_refusals():
    f = torch.zeros(2, ref.frame_bytes(4, 6, "420jpeg"), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv_to_rgb_u8(f, 4, 6, "420p10")
    with pytest.raises(ValueError, match="matrix"):
        ops.yuv_to_rgb_u8(f, 4, 6, "420jpeg", matrix="bt2020")
    with pytest.raises(ValueError, match="frames must be"):
        ops.yuv_to_rgb_u8(f, 4, 8, "420jpeg")
    with pytest.raises(ValueError, match="frames must be"):
        ops.yuv_to_rgb_u8(f.cpu(), 4, 6, "420jpeg")
    with pytest.raises(ValueError, match="limits"):
        ops.yuv_to_rgb_u8(f, 0, 6, "420jpeg")
    x = torch.zeros(2, 4, 6, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="uint8"):
        ops.rgb_to_yuv_u8(x.float(), "420jpeg")
    with pytest.raises(ValueError, match="out holds"):
        ops.rgb_to_yuv_u8(x, "420jpeg", out=f[:1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.rgb_to_yuv_u8(x.cpu(), "420jpeg")
    grey = ops.rgb_to_yuv_u8(torch.full((4, 6, 3), 200, dtype=torch.uint8, device=DEV), "420jpeg", "bt601", True)
    assert grey[:24].tolist() == [200] * 24 and grey[24:].tolist() == [128] * 12
