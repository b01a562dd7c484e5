"""Deep YCbCr <-> float RGB on the device (cfen_yuv16_to_rgb_f32, cfen_rgb_f32_to_yuv16; ops.yuv16_to_rgb_f32, ops.rgb_f32_to_yuv16) against the
numpy restatement tests/yuv16_ref.py.  The sums are integers and each float is one IEEE division, so every comparison is bitwise."""
import ctypes

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, yuv
import cabi_ledger
import guarded
import yuv16_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (H, W).  3 x 5 and 17 x 33 have an odd number of pixels: the second and third float plane and the chroma planes leave the 16- and 8-byte
# boundaries.  130 x 259: rows of odd length, more than one block per frame both ways
SIZES = [(1, 1), (2, 2), (3, 5), (17, 33), (64, 64), (130, 259)]
TABLES = [(10, "bt601", False), (16, "bt709", True)]
OTHER_DEPTHS = [(9, "bt709", True), (12, "bt601", False), (14, "bt709", False)]
SPECIAL = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, 0.25, -0.75)
_CACHE = {}


def case(H, W, chroma, depth, matrix, full):
    """(frames (2, nbytes) uint8: random samples -- out-of-gamut YCbCr, and samples above top below 16 bits --, their float RGB (2,3,H,W); rgb
    (2,3,H,W) float32: values on and off the grid of levels, exact halves, values past +-1, NaN and infinities --, its frames): computed once"""
    key = (H, W, chroma, depth, matrix, full)
    if key not in _CACHE:
        rs = np.random.RandomState(hash((H, W, len(chroma), depth)) % 2 ** 31)
        oy, peak, c, top = ref.levels(depth, full)
        ns = ref.frame_samples(H, W, chroma)
        v = rs.randint(0, top + 1, (2, ns))
        v[1, :min(ns, 6)] = (0, top, 65535, min(top + 1, 65535), oy, c)[:min(ns, 6)]           # above top: read as top
        frames = np.stack([ref.payload(f) for f in v])
        rgb = rs.uniform(-1.3, 1.3, (2, 3, H, W)).astype(np.float32)
        grid = (2 * rs.randint(0, peak + 1, rgb.shape) / np.float32(peak) - 1).astype(np.float32)
        halves = ((2 * rs.randint(0, peak, rgb.shape) + 1) / np.float32(peak) - 1).astype(np.float32)      # at or beside k + 0.5 levels
        pick = rs.randint(0, 3, rgb.shape)
        rgb = np.where(pick == 0, rgb, np.where(pick == 1, grid, halves)).astype(np.float32)
        flat = rgb[1].reshape(-1)
        flat[:min(flat.size, len(SPECIAL))] = SPECIAL[:min(flat.size, len(SPECIAL))]
        want_rgb = np.stack([ref.yuv_to_rgb(f, H, W, chroma, depth, matrix, full) for f in frames])
        want_frames = np.stack([ref.rgb_to_yuv(x, chroma, depth, matrix, full) for x in rgb])
        for a in (frames, rgb, want_rgb, want_frames):
            a.setflags(write=False)
        _CACHE[key] = (frames, want_rgb, rgb, want_frames)
    return _CACHE[key]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def bits(t):
    """float32 values as their bit patterns (a numpy array or a tensor)"""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _both(H, W, chroma, depth, matrix, full):
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, depth, matrix, full)
    got = ops.yuv16_to_rgb_f32(dev(frames), H, W, chroma, depth, matrix, full)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, H, W)
    bad = int((bits(got) != bits(want_rgb)).sum())
    print("to rgb: %d of %d floats differ%s" % (bad, want_rgb.size, " (first at %s)" % (np.argwhere(bits(got) != bits(want_rgb))[:4].tolist(),) if bad else ""))
    assert bad == 0
    back = ops.rgb_f32_to_yuv16(dev(rgb), chroma, depth, matrix, full)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (2, ref.frame_bytes(H, W, chroma))
    bad = int((back.cpu().numpy() != want_frames).sum())
    print("to yuv: %d of %d bytes differ%s" % (bad, want_frames.size, " (first at %s)" % (np.argwhere(back.cpu().numpy() != want_frames)[:4].tolist(),) if bad else ""))
    assert bad == 0
    return want_rgb


def test_frame_bytes():
    q = _lib.load().cfen_yuv16_frame_bytes
    for H, W in SIZES + [(65536, 65536), (1, 65536)]:
        for chroma, code in yuv.CHROMA.items():
            assert q(H, W, code) == ref.frame_bytes(H, W, chroma) == yuv.frame_bytes(H, W, chroma, 10)
    assert q(0, 4, 0) == 0 and q(4, 0, 0) == 0 and q(65537, 4, 0) == 0 and q(4, 65537, 0) == 0 and q(4, 4, 5) == 0 and q(4, 4, -1) == 0


@pytest.mark.parametrize("depth,matrix,full", TABLES)
@pytest.mark.parametrize("chroma", ref.CHROMAS)
@pytest.mark.parametrize("H,W", SIZES)
def test_both_directions_equal_the_restatement(H, W, chroma, depth, matrix, full):
    want_rgb = _both(H, W, chroma, depth, matrix, full)
    if (H, W) == (130, 259):                                            # the clamps are hit
        assert (want_rgb == -1).any() and (want_rgb == 1).any()


@pytest.mark.parametrize("depth,matrix,full", OTHER_DEPTHS)
@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_the_other_depths(chroma, depth, matrix, full):
    _both(17, 33, chroma, depth, matrix, full)


@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_batch_stream_offset_and_stride_do_not_change_a_bit(chroma):
    H, W, depth, matrix, full = 17, 33, 10, "bt601", False
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, depth, matrix, full)
    n, nf = frames.shape[1], 3 * 3 * H * W
    f3 = dev(np.concatenate([frames, frames[:1]]))
    x3 = dev(np.concatenate([rgb, rgb[:1]]))
    got3 = ops.yuv16_to_rgb_f32(f3, H, W, chroma, depth, matrix, full)
    back3 = ops.rgb_f32_to_yuv16(x3, chroma, depth, matrix, full)
    assert np.array_equal(bits(got3), bits(np.concatenate([want_rgb, want_rgb[:1]])))
    assert np.array_equal(back3.cpu().numpy(), np.concatenate([want_frames, want_frames[:1]]))
    one = ops.yuv16_to_rgb_f32(f3[1].clone(), H, W, chroma, depth, matrix, full)                 # a frame alone (1-D in, (3,H,W) out)
    assert tuple(one.shape) == (3, H, W) and np.array_equal(bits(one), bits(got3[1]))
    one = ops.rgb_f32_to_yuv16(x3[1].clone(), chroma, depth, matrix, full)
    assert tuple(one.shape) == (n,) and torch.equal(one, back3[1])
    assert torch.equal(ops.rgb_f32_to_yuv16(x3.half().float().half(), chroma, depth, matrix, full),           # float16 images: .float()
                       ops.rgb_f32_to_yuv16(x3.half().float(), chroma, depth, matrix, full))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a, b = ops.yuv16_to_rgb_f32(f3, H, W, chroma, depth, matrix, full), ops.rgb_f32_to_yuv16(x3, chroma, depth, matrix, full)
    side.synchronize()
    assert np.array_equal(bits(a), bits(got3)) and torch.equal(b, back3)
    # frames frame_bytes + 6 apart, at byte offsets 0 and 2 of a larger buffer; float tensors at element offsets 0 .. 3
    stride = n + 6
    for boff, eoff in ((0, 1), (2, 2), (2, 3), (2, 0)):
        fb = torch.full((3 * stride + 8,), 0xAA, dtype=torch.uint8, device=DEV)
        fv = fb[boff:boff + 3 * stride].view(3, stride)[:, :n]
        fv.copy_(f3)
        xb = torch.zeros(nf + 8, dtype=torch.float32, device=DEV)
        xv = xb[eoff:eoff + nf].view(3, 3, H, W)
        xv.copy_(x3)
        assert fv.data_ptr() % 8 == boff and xv.data_ptr() % 16 == 4 * eoff and fv.stride(0) == stride
        ob = torch.zeros(nf + 8, dtype=torch.float32, device=DEV)
        got = ops.yuv16_to_rgb_f32(fv, H, W, chroma, depth, matrix, full, out=ob[eoff:eoff + nf].view(3, 3, H, W))
        assert np.array_equal(bits(got), bits(got3)), (boff, eoff)
        assert float(ob[:eoff].abs().sum()) == 0 and float(ob[eoff + nf:].abs().sum()) == 0
        assert np.array_equal(bits(ops.yuv16_to_rgb_f32(fv, H, W, chroma, depth, matrix, full)), bits(got3)), (boff, eoff)       # aligned output
        yb = torch.full((3 * stride + 8,), 0x55, dtype=torch.uint8, device=DEV)
        yv = yb[boff:boff + 3 * stride].view(3, stride)[:, :n]
        ops.rgb_f32_to_yuv16(xv, chroma, depth, matrix, full, out=yv)
        assert torch.equal(yv, back3), (boff, eoff)
        gaps = yb[boff:boff + 3 * stride].view(3, stride)[:, n:]
        assert bool((gaps == 0x55).all()) and bool((yb[:boff] == 0x55).all()) and bool((yb[boff + 3 * stride:] == 0x55).all())
        assert torch.equal(ops.rgb_f32_to_yuv16(x3, chroma, depth, matrix, full, out=yv), back3), (boff, eoff)                   # aligned images


# ---- guard bands -----------------------------------------------------------------------------------------------------------------------
def test_guard_bands_yuv16():
    """inputs between 0xff bands (NaN to a float read past an end), outputs prefilled 0xff, zeros and random bytes between random bands: no band
    changes, every payload byte and every float is written (the result is the unguarded call's whatever the prefill), the gap between two frames
    keeps its bytes"""
    lib = _lib.load()
    for (H, W), chroma, depth in (((17, 33), "420jpeg", 10), ((130, 259), "420mpeg2", 16), ((3, 5), "422", 12), ((17, 33), "444", 10), ((2, 2), "mono", 16),
                                  ((1, 1), "420mpeg2", 10)):
        matrix, full = "bt709", True
        code = yuv.CHROMA[chroma]
        frames, want_rgb, rgb, want_frames = case(H, W, chroma, depth, matrix, full)
        n = lib.cfen_yuv16_frame_bytes(H, W, code)
        assert n == frames.shape[1]
        stride = n + 6
        fwd, inv, _ = yuv.tables(matrix, full, shift=20)
        oy, peak, _ = yuv.levels(depth, full)
        strided = np.zeros((2, stride), dtype=np.uint8)
        strided[:, :n] = frames
        gin = guarded.guarded_copy(dev(strided))
        gout = guarded.guarded_empty((2, 3, H, W), torch.float32, DEV)
        for fill in guarded.FILLS:
            guarded.refill(gout, fill)
            _lib.check(lib.cfen_yuv16_to_rgb_f32(_lib.ptr(gin), stride, 2, H, W, code, ops.yuv16_table(inv, oy, peak, depth), _lib.ptr(gout),
                                                 _lib.current_stream()), "yuv16_to_rgb_f32")
            torch.cuda.synchronize()
            guarded.check_bands(gin, gout)
            assert np.array_equal(bits(gout), bits(want_rgb)), (H, W, chroma, fill)
        gin = guarded.guarded_copy(dev(rgb))
        gout = guarded.guarded_empty((2, stride), torch.uint8, DEV)
        for fill in guarded.FILLS:
            guarded.refill(gout, fill)
            before = gout.clone()
            _lib.check(lib.cfen_rgb_f32_to_yuv16(_lib.ptr(gin), 2, H, W, code, ops.yuv16_table(fwd, oy, peak, depth), _lib.ptr(gout), stride,
                                                 _lib.current_stream()), "rgb_f32_to_yuv16")
            torch.cuda.synchronize()
            guarded.check_bands(gin, gout)
            assert np.array_equal(gout[:, :n].cpu().numpy(), want_frames), (H, W, chroma, fill)
            assert torch.equal(gout[:, n:], before[:, n:]), (H, W, chroma, fill)                 # the stride gap
        assert lib.cfen_yuv16_frame_bytes(H, W, code) == ref.frame_bytes(H, W, chroma)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    lib = _lib.load()
    H, W, chroma, depth = 3, 5, "420jpeg", 10
    frames, want_rgb, rgb, want_frames = case(H, W, chroma, depth, "bt601", False)
    n = frames.shape[1]
    fwd, inv, _ = yuv.tables("bt601", False, shift=20)
    oy, peak, _ = yuv.levels(depth, False)
    f, x = dev(frames), dev(rgb)
    out_rgb = torch.full((2, 3, H, W), 7.0, dtype=torch.float32, device=DEV)
    out_f = torch.full((2, n), 7, dtype=torch.uint8, device=DEV)
    z = ctypes.c_void_p(0)

    def table(t, reserved=None, coef=None, **fields):
        c = ops.yuv16_table(t, fields.get("oy", oy), fields.get("peak", peak), fields.get("depth", depth))
        if reserved is not None:
            c.reserved[reserved] = 1
        if coef is not None:
            c.coef[4] = coef
        return c
    to_rgb = ("frames", "stride", "B", "H", "W", "chroma", "table", "rgb")
    to_yuv = ("rgb", "B", "H", "W", "chroma", "table", "frames", "stride")
    good = dict(frames=_lib.ptr(f), stride=n, B=2, H=H, W=W, chroma=0, table=table(inv), rgb=_lib.ptr(out_rgb))
    good2 = dict(good, frames=_lib.ptr(out_f), rgb=_lib.ptr(x), table=table(fwd))

    def bad_cases(g, t):
        return [("frames", z, b"null pointer"), ("rgb", z, b"null pointer"), ("B", 0, b"B = 0"), ("B", 65536, b"B = 65536"), ("H", 0, b"H = 0"),
                ("W", 65537, b"W = 65537"), ("H", -3, b"H = -3"), ("chroma", 5, b"unknown chroma = 5"), ("chroma", -1, b"unknown chroma = -1"),
                ("table", table(t, depth=8), b"depth outside"), ("table", table(t, depth=17), b"depth outside"), ("table", table(t, peak=0), b"peak outside"),
                ("table", table(t, peak=1024), b"peak outside"), ("table", table(t, oy=-1), b"luma_offset outside"), ("table", table(t, oy=1024), b"luma_offset outside"),
                ("table", table(t, coef=(1 << 22) + 1), b"coefficients outside"), ("table", table(t, coef=-(1 << 22) - 1), b"coefficients outside"),
                ("table", table(t, reserved=0), b"reserved word"), ("table", table(t, reserved=3), b"reserved word"),
                ("stride", n - 2, b"frame_stride"), ("stride", n + 1, b"odd"), ("frames", cabi_ledger.off(g["frames"], 1), b"odd"),
                ("rgb", cabi_ledger.off(g["rgb"], 2), b"4-byte aligned"), ("rgb", cabi_ledger.off(g["rgb"], 1), b"4-byte aligned")]
    for key, value, what in bad_cases(good, inv):
        rc = lib.cfen_yuv16_to_rgb_f32(*[dict(good, **{key: value})[k] for k in to_rgb], _lib.current_stream())
        err = lib.cfen_last_error()
        assert rc == -1 and b"yuv16_to_rgb_f32" in err and what in err, (key, rc, err)
    for key, value, what in bad_cases(good2, fwd):
        rc = lib.cfen_rgb_f32_to_yuv16(*[dict(good2, **{key: value})[k] for k in to_yuv], _lib.current_stream())
        err = lib.cfen_last_error()
        assert rc == -1 and b"rgb_f32_to_yuv16" in err and what in err, (key, rc, err)
    torch.cuda.synchronize()
    assert bool((out_rgb == 7).all()) and bool((out_f == 7).all())
    _lib.check(lib.cfen_yuv16_to_rgb_f32(*[good[k] for k in to_rgb], _lib.current_stream()), "yuv16_to_rgb_f32")
    _lib.check(lib.cfen_rgb_f32_to_yuv16(*[good2[k] for k in to_yuv], _lib.current_stream()), "rgb_f32_to_yuv16")
    torch.cuda.synchronize()
    assert np.array_equal(bits(out_rgb), bits(want_rgb)) and np.array_equal(out_f.cpu().numpy(), want_frames)


def test_python_side_refusals():
    f = torch.zeros(2, ref.frame_bytes(4, 6, "420jpeg"), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv16_to_rgb_f32(f, 4, 6, "420p10", 10)
    with pytest.raises(ValueError, match="depth"):
        ops.yuv16_to_rgb_f32(f, 4, 6, "420jpeg", 8)
    with pytest.raises(ValueError, match="depth"):
        ops.yuv16_to_rgb_f32(f, 4, 6, "420jpeg", 17)
    with pytest.raises(ValueError, match="matrix"):
        ops.yuv16_to_rgb_f32(f, 4, 6, "420jpeg", 10, matrix="bt2020")
    with pytest.raises(ValueError, match="frames must be"):
        ops.yuv16_to_rgb_f32(f, 4, 8, "420jpeg", 10)
    with pytest.raises(ValueError, match="frames must be"):
        ops.yuv16_to_rgb_f32(f.cpu(), 4, 6, "420jpeg", 10)
    with pytest.raises(ValueError, match="limits"):
        ops.yuv16_to_rgb_f32(f, 0, 6, "420jpeg", 10)
    with pytest.raises(ValueError, match="out must be"):
        ops.yuv16_to_rgb_f32(f, 4, 6, "420jpeg", 10, out=torch.zeros(2, 4, 6, 3, dtype=torch.float32, device=DEV))
    x = torch.zeros(2, 3, 4, 6, dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        ops.rgb_f32_to_yuv16(x.double(), "420jpeg", 10)
    with pytest.raises(ValueError, match="float32"):
        ops.rgb_f32_to_yuv16(x.permute(0, 2, 3, 1).contiguous(), "420jpeg", 10)
    with pytest.raises(ValueError, match="out holds"):
        ops.rgb_f32_to_yuv16(x, "420jpeg", 10, out=f[:1])
    with pytest.raises(ValueError, match="contiguous"):
        ops.rgb_f32_to_yuv16(x.cpu(), "420jpeg", 10)
    grey = ops.rgb_f32_to_yuv16(torch.full((3, 4, 6), 0.5, dtype=torch.float32, device=DEV), "420jpeg", 10, "bt601", True)
    assert ref.samples(grey.cpu().numpy()).tolist() == [767] * 24 + [512] * 12          # rint(0.75 * 1023) = 767
