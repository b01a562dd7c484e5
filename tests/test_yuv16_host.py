"""Host side of the deep (9 to 16 bits per sample) YCbCr <-> float RGB extension: the 2^-20 tables of cfen_vit_dehazing_amd/yuv.py against their
known answers and the float64 formulas, the restatement tests/yuv16_ref.py against a double loop over pixels, the float edge cases, the deep tags
of the y4m reader (cfen_vit_dehazing_amd/video.py), the ledger of include/cfen_yuv16.h, and the banding argument in numbers.

Bars (include/cfen_yuv16.h; 2 * 10^6 seeded triples per case):
  integer forward / inverse against float64   <= 0.5 + 3 top 2^-21: three coefficients rounded to 2^-21 each times at most top, and the final
                                              rounding (0.594 at 16 bits, 0.501 at 10)
  RGB -> YCbCr -> RGB at 4:4:4                <= 2 levels limited range, <= 1 full range
  greys                                       <= 1 limited, 0 full; R = G = B gives Cb = Cr = centre, white and black their exact codes"""
import io
import os
import re

import numpy as np
import pytest

from cfen_vit_dehazing_amd import video, yuv
import cabi_ledger
import yuv16_ref as ref
import yuv_ref as ref8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
TRIPLES = 2 * 10 ** 6


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_the_14_bit_tables_are_unchanged(matrix, full):
    wf, wi, woy = ref8.table(matrix, full)
    for got in (yuv.tables(matrix, full), yuv.tables(matrix, full, shift=14), yuv.tables(matrix, full, 14)):
        fwd, inv, oy = got
        assert fwd.dtype == np.int32 and inv.dtype == np.int32
        assert fwd.tolist() == wf.tolist() and inv.tolist() == wi.tolist() and oy == woy
    with pytest.raises(ValueError, match="shift"):
        yuv.tables(matrix, full, shift=16)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_the_20_bit_tables_meet_their_row_sums_and_known_answers(matrix, full):
    fwd, inv, oy = yuv.tables(matrix, full, shift=20)
    wf, wi = ref.table(matrix, full)
    assert fwd.dtype == np.int32 and inv.dtype == np.int32 and fwd.shape == (3, 3) and inv.shape == (3, 3) and oy == (0 if full else 16)
    assert fwd.tolist() == wf.tolist() and inv.tolist() == wi.tolist()
    assert int(fwd[0].sum()) == round((255 if full else 219) / 255 * 2 ** 20) and fwd[1].sum() == 0 and fwd[2].sum() == 0
    assert int(np.abs(fwd).max()) <= 1 << 22 and int(np.abs(inv).max()) <= 1 << 22          # the range the C functions accept
    ff, fi, _ = yuv.float_matrices(matrix, full)
    assert np.abs(fwd - ff * 2 ** 20).max() <= 1.5 and np.abs(inv - fi * 2 ** 20).max() <= 0.5


def test_levels_and_frame_bytes():
    assert yuv.DEPTHS == ref.DEPTHS == (9, 10, 12, 14, 16)
    for d in range(9, 17):
        for full in (False, True):
            oy, peak, c, top = ref.levels(d, full)
            assert yuv.levels(d, full) == (oy, peak, c)
            assert (oy, peak) == ((0, 2 ** d - 1) if full else (16 << (d - 8), 255 << (d - 8))) and c == 2 ** (d - 1) and top == 2 ** d - 1
        for chroma in ref.CHROMAS:
            assert yuv.frame_bytes(5, 7, chroma, d) == 2 * yuv.frame_bytes(5, 7, chroma) == ref.frame_bytes(5, 7, chroma)
    assert yuv.levels(8, False) == (16, 255, 128) and yuv.frame_bytes(5, 7, "444", 8) == yuv.frame_bytes(5, 7, "444") == 105
    for bad in (7, 17, 10.5, "10"):
        with pytest.raises(ValueError, match="depth"):
            yuv.frame_bytes(5, 7, "444", bad)
        with pytest.raises(ValueError, match="depth"):
            yuv.levels(bad, False)


@pytest.mark.parametrize("matrix,full", [("bt601", False), ("bt709", True)])
@pytest.mark.parametrize("depth", [9, 10, 12, 16])
def test_bounds_on_seeded_triples(depth, matrix, full):
    fwd, inv = ref.table(matrix, full)
    assert [t.tolist() for t in yuv.tables(matrix, full, shift=20)[:2]] == [fwd.tolist(), inv.tolist()]
    ff, fi, _ = yuv.float_matrices(matrix, full)
    oy, peak, c, top = ref.levels(depth, full)
    off = np.array([oy, c, c], dtype=np.float64)
    bound = 0.5 + 3 * top * 2.0 ** -21
    rs = np.random.RandomState(1000 * depth + len(matrix) + int(full))
    q = rs.randint(0, peak + 1, (TRIPLES, 3)).astype(np.int64)
    q[:4] = ((0, 0, 0), (peak, peak, peak), (peak, 0, 0), (0, 0, peak))
    ycc = ref.forward_pixels(q, fwd, depth, full)
    worst_f = float(np.abs(ycc - np.clip(q @ ff.T + off, 0, top)).max())
    back = ref.inverse_pixels(ycc, inv, depth, full)
    worst_rt = int(np.abs(back - q).max())
    anyc = rs.randint(0, top + 1, (TRIPLES, 3)).astype(np.int64)                # read as (Y, Cb, Cr): out of gamut included
    rgb = ref.inverse_pixels(anyc, inv, depth, full)
    worst_i = float(np.abs(rgb - np.clip((anyc - off) @ fi.T, 0, peak)).max())
    g = np.arange(0, peak + 1, dtype=np.int64)
    g = g if g.size <= TRIPLES else g[rs.randint(0, g.size, TRIPLES)]
    grey = ref.forward_pixels(np.stack([g, g, g], axis=-1), fwd, depth, full)
    worst_grey = int(np.abs(ref.inverse_pixels(grey, inv, depth, full) - g[:, None]).max())
    print("%d bits %s %s: forward %.4f, inverse %.4f (bound %.4f), round trip %d, greys %d" % (depth, matrix, "full" if full else "limited", worst_f,
                                                                                             worst_i, bound, worst_rt, worst_grey))
    assert (grey[:, 1] == c).all() and (grey[:, 2] == c).all()                  # R = G = B gives Cb = Cr = the centre exactly
    s = depth - 8
    assert ycc[0].tolist() == [0 if full else 16 << s, c, c] and ycc[1].tolist() == [top if full else 235 << s, c, c]
    assert worst_f <= bound and worst_i <= bound
    assert worst_rt <= (1 if full else 2)
    assert worst_grey <= (0 if full else 1)


# ---- the restatement against a double loop over pixels -----------------------------------------------------------------------------------
def _to_rgb_loops(frame, H, W, chroma, depth, matrix, full):
    _, inv = ref.table(matrix, full)
    oy, peak, c, top = ref.levels(depth, full)
    y, cb, cr = ref.split(frame, H, W, chroma)
    if chroma != "mono":
        cb = ref8.upsample_loops(np.minimum(cb.astype(np.int64), top), H, W, chroma)
        cr = ref8.upsample_loops(np.minimum(cr.astype(np.int64), top), H, W, chroma)
    out = np.zeros((3, H, W), dtype=np.float32)
    for r in range(H):
        for x in range(W):
            v = (min(int(y[r, x]), top) - oy, (int(cb[r, x]) if chroma != "mono" else c) - c, (int(cr[r, x]) if chroma != "mono" else c) - c)
            for k in range(3):
                q = min(max((sum(int(inv[k, n]) * v[n] for n in range(3)) + (1 << 19)) >> 20, 0), peak)
                out[k, r, x] = np.float32(2 * q - peak) / np.float32(peak)
    return out


def _to_yuv_loops(rgb, chroma, depth, matrix, full):
    fwd, _ = ref.table(matrix, full)
    oy, peak, c, top = ref.levels(depth, full)
    _, H, W = rgb.shape
    d = np.zeros((3, H, W), dtype=np.int64)
    for r in range(H):
        for x in range(W):
            q = []
            for k in range(3):
                t = np.float32(rgb[k, r, x]) * np.float32(0.5) + np.float32(0.5)
                t = np.float32(0.0) if not t >= 0 else min(t, np.float32(1.0))
                q.append(int(np.rint(np.float32(t) * np.float32(peak))))
            for k, o in enumerate((oy, c, c)):
                d[k, r, x] = min(max((sum(int(fwd[k, n]) * q[n] for n in range(3)) + (o << 20) + (1 << 19)) >> 20, 0), top)
    planes = [d[0]] + ([ref8.downsample_loops(d[1], chroma), ref8.downsample_loops(d[2], chroma)] if chroma != "mono" else [])
    return ref.payload(np.concatenate([p.reshape(-1) for p in planes]))


@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_loops_agree_with_the_vectorised_restatement(chroma):
    rs = np.random.RandomState(5)
    for (H, W), depth, matrix, full in (((3, 5), 10, "bt601", False), ((8, 8), 16, "bt709", True), ((3, 5), 12, "bt709", True)):
        top = 2 ** depth - 1
        v = rs.randint(0, top + 1, ref.frame_samples(H, W, chroma))
        v[:2] = (65535, top)                                                   # a stored value above top reads as top
        frame = ref.payload(v)
        assert frame.size == ref.frame_bytes(H, W, chroma)
        got = ref.yuv_to_rgb(frame, H, W, chroma, depth, matrix, full)
        assert got.dtype == np.float32 and got.shape == (3, H, W)
        assert np.array_equal(got.view(np.uint32), _to_rgb_loops(frame, H, W, chroma, depth, matrix, full).view(np.uint32))
        rgb = rs.uniform(-1.2, 1.2, (3, H, W)).astype(np.float32)
        rgb[0, 0, :3] = (np.nan, np.inf, -np.inf)
        back = ref.rgb_to_yuv(rgb, chroma, depth, matrix, full)
        assert back.dtype == np.uint8 and back.size == ref.frame_bytes(H, W, chroma)
        assert np.array_equal(back, _to_yuv_loops(rgb, chroma, depth, matrix, full))
        assert int(ref.samples(back).max()) <= top


@pytest.mark.parametrize("chroma", [c for c in ref.CHROMAS if c != "mono"])
def test_constant_chroma_survives_up_and_down_exactly(chroma):
    for H, W in ((1, 1), (3, 5), (8, 8)):
        hc, wc = ref.chroma_shape(H, W, chroma)
        for v in (0, 1, 511, 512, 32768, 65534, 65535):
            up = ref8.upsample(np.full((hc, wc), v), H, W, chroma)
            assert up.shape == (H, W) and (up == v).all()
            down = ref8.downsample(np.full((H, W), v), chroma)
            assert down.shape == (hc, wc) and (down == v).all()
    # a grey float image: chroma planes at the centre, and it comes back within a level
    for depth, full in ((10, False), (16, True)):
        oy, peak, c, top = ref.levels(depth, full)
        g = np.linspace(-1, 1, 15, dtype=np.float32).reshape(3, 5)
        frame = ref.rgb_to_yuv(np.stack([g, g, g]), chroma, depth, "bt709", full)
        assert (ref.samples(frame)[15:] == c).all()
        back = ref.yuv_to_rgb(frame, 3, 5, chroma, depth, "bt709", full)
        assert np.abs((back[0] - g) * peak / 2).max() <= (0.5 if full else 1.5) + 1e-3


def test_float_edges_half_to_even_nan_and_clamps():
    # limited 9 bits: peak 510.  x = -0.5 -> t = 0.25 -> 127.5 -> 128;  x = 0.5 -> t = 0.75 -> 382.5 -> 382: both to the even neighbour
    assert ref.quantise(np.float32([-0.5, 0.5, 0.0]), 510).tolist() == [128, 382, 255]
    # full 10 and 16 bits: x = 0 -> t = 0.5 -> 511.5 -> 512 and 32767.5 -> 32768
    assert ref.quantise(np.float32([0.0]), 1023).tolist() == [512] and ref.quantise(np.float32([0.0]), 65535).tolist() == [32768]
    x = np.float32([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.5, -1.5, 3e38, -3e38, 1e-45, -0.0])
    assert ref.quantise(x, 1020).tolist() == [0, 1020, 0, 1020, 0, 1020, 0, 1020, 0, 510, 510]
    # through a whole frame: NaN is black, +inf white, at 10 bits limited 64 and 940
    rgb = np.zeros((3, 1, 4), dtype=np.float32)
    rgb[:, 0, 0], rgb[:, 0, 1], rgb[:, 0, 2], rgb[:, 0, 3] = np.nan, np.inf, -7.0, 7.0
    assert ref.samples(ref.rgb_to_yuv(rgb, "mono", 10, "bt601", False)).tolist() == [64, 940, 64, 940]
    # rounding, where tensor2im would truncate: 0.999 of a level above a code still gives that code + 1
    assert ref.quantise(np.float32([2 * (100.9 / 1020) - 1]), 1020).tolist() == [101]
    # the floats the other way: 0 and peak are exactly -1 and 1, the division is float32's
    assert ref.to_float(np.array([0, 1020, 510, 1]), 1020).tolist() == [-1.0, 1.0, 0.0, float(np.float32(-1018) / np.float32(1020))]


# ---- reader and writer -----------------------------------------------------------------------------------------------------------------
DEEP_TAGS = [("C%sp%d" % (c, d), {"420": "420mpeg2"}.get(c, c), d) for c in ("420", "422", "444") for d in ref.DEPTHS] + \
            [("Cmono%d" % d, "mono", d) for d in (9, 10, 12, 16)]


@pytest.mark.parametrize("tag,chroma,depth", DEEP_TAGS)
def test_every_deep_tag_is_read_with_max_depth_16_and_refused_without(tag, chroma, depth):
    header = ("YUV4MPEG2 W6 H4 F25:1 Ip A1:1 %s XCOLORRANGE=FULL\n" % tag).encode()
    assert ref.y4m_header(6, 4, chroma, depth, extra=("XCOLORRANGE=FULL",)) == header
    rs = np.random.RandomState(depth)
    frames = [ref.payload(rs.randint(0, 2 ** depth, ref.frame_samples(4, 6, chroma))) for _ in range(2)]
    data = ref.y4m_bytes(frames, 6, 4, chroma, depth, header=header)
    r = video.Y4MReader(io.BytesIO(data), max_depth=16)
    assert (r.width, r.height, r.chroma, r.depth, r.color_range, r.header) == (6, 4, chroma, depth, "full", header)
    assert r.frame_bytes == ref.frame_bytes(4, 6, chroma) == 2 * ref8.frame_bytes(4, 6, chroma) and r.check_whole_file() == 2
    assert r.read_frame() == frames[0].tobytes() and r.read_frame() == frames[1].tobytes() and r.read_frame() is None
    info = video.parse_header(header, max_depth=16)
    assert (info["chroma"], info["depth"]) == (chroma, depth)
    for kw in ({}, {"max_depth": 8}):
        with pytest.raises(video.Y4MError, match=re.escape(tag)):
            video.Y4MReader(io.BytesIO(data), **kw)
        with pytest.raises(video.Y4MError, match=re.escape(tag)):
            video.parse_header(header, **kw)


def test_what_no_tool_writes_stays_refused_and_8_bit_streams_read_as_before():
    for tag in ("Cmono14", "C420p11", "C420p8", "C444p17", "C420jpegp10", "C420paldv"):
        with pytest.raises(video.Y4MError, match=re.escape(tag)):
            video.Y4MReader(io.BytesIO(("YUV4MPEG2 W6 H4 %s\n" % tag).encode()), max_depth=16)
    for header, chroma in ((b"YUV4MPEG2 W6 H4 C420jpeg\n", "420jpeg"), (b"YUV4MPEG2 W6 H4\n", "420jpeg"), (b"YUV4MPEG2 W6 H4 Cmono\n", "mono")):
        r = video.Y4MReader(io.BytesIO(header), max_depth=16)
        assert (r.chroma, r.depth, r.frame_bytes) == (chroma, 8, ref8.frame_bytes(4, 6, chroma))
        assert video.Y4MReader(io.BytesIO(header)).depth == 8


def test_a_422p12_stream_round_trips_byte_for_byte_and_a_cut_frame_is_named(tmp_path):
    rs = np.random.RandomState(12)
    frames = [ref.payload(rs.randint(0, 4096, ref.frame_samples(5, 7, "422"))) for _ in range(3)]
    data = ref.y4m_bytes(frames, 7, 5, "422", 12)
    assert data.startswith(b"YUV4MPEG2 W7 H5 F25:1 Ip A1:1 C422p12\n")
    (tmp_path / "a.y4m").write_bytes(data)
    r = video.Y4MReader(str(tmp_path / "a.y4m"), max_depth=16)
    assert r.check_whole_file() == 3 and r.frame_bytes == 2 * (35 + 2 * 20)
    w = video.Y4MWriter(str(tmp_path / "b.y4m"), r.header)
    buf = bytearray(r.frame_bytes)
    while r.read_frame_into(buf):
        w.write_frame(buf)
    w.close()
    r.close()
    assert (tmp_path / "b.y4m").read_bytes() == data and r.frames_read == 3 and w.frames_written == 3
    n = len(frames[0])
    for cut, where in ((5, "frame 2"), (n + 6 + 3, "frame 1"), (n + 3, "frame 2")):
        r = video.Y4MReader(io.BytesIO(data[:-cut]), max_depth=16)
        with pytest.raises(video.Y4MError, match=where + " is cut short"):
            r.check_whole_file()
        with pytest.raises(video.Y4MError, match=where + " is cut short"):
            while r.read_frame() is not None:
                pass


def test_deep_streams_refuse_the_uint8_machinery_by_name():
    class Opt:
        fit = temporal = eval_noref = eval_flicker = False
    video.refuse_deep_flags(Opt(), "C420p10")
    for flag in video.DEEP_REFUSED:
        o = Opt()
        setattr(o, flag, True)
        with pytest.raises(video.Y4MError) as e:
            video.refuse_deep_flags(o, "C420p10")
        assert "C420p10" in str(e.value) and "--" + flag + " is given" in str(e.value)
    assert video.DEEP_REFUSED == ("fit", "temporal", "eval_noref", "eval_flicker")


# ---- the header's ledger ---------------------------------------------------------------------------------------------------------------
def test_every_function_of_the_yuv16_header_is_bound_and_guard_band_tested():
    import ctypes
    from cfen_vit_dehazing_amd import _lib
    fns = {"cfen_yuv16_frame_bytes": 3, "cfen_yuv16_to_rgb_f32": 9, "cfen_rgb_f32_to_yuv16": 9}
    cabi_ledger.check_header_bound("cfen_yuv16.h", fns)
    assert ctypes.sizeof(_lib.Yuv16TableC) == 64 and [n for n, _ in _lib.Yuv16TableC._fields_] == ["coef", "luma_offset", "peak", "depth", "reserved"]
    cabi_ledger.check_guard_band_test_calls("test_hip_yuv16.py", "test_guard_bands_yuv16", fns)
    lib = _lib.load()
    assert lib.cfen_abi_version() == 1 and len(_lib.SIGNATURES) == 68
    for chroma, code in yuv.CHROMA.items():                                    # host code only: no device is touched
        assert lib.cfen_yuv16_frame_bytes(5, 7, code) == ref.frame_bytes(5, 7, chroma) == 2 * lib.cfen_yuv_frame_bytes(5, 7, code)
    assert lib.cfen_yuv16_frame_bytes(0, 4, 0) == 0 and lib.cfen_yuv16_frame_bytes(4, 65537, 0) == 0 and lib.cfen_yuv16_frame_bytes(4, 4, 5) == 0
    text = open(os.path.join(ROOT, "include", "cfen_yuv16.h")).read()
    for words in ("units of 2^-20", "All sums are 64-bit integers", "half to even", "one correctly rounded fp32 division", "tensor2im"):
        assert words in text, words


# ---- why: banding ----------------------------------------------------------------------------------------------------------------------
def test_a_dehazed_grey_ramp_bands_at_most_half_as_much_at_10_bits():
    """A grey ramp from 0.6 to 0.9 over 512 columns, stored as 4:4:4 limited-range YCbCr, dehazed exactly (J = (I - A) / t + A with t = 0.25,
    A = 0.95) and stored again at the depth it came in.  The largest step between neighbouring columns of the stored luma, as a fraction of full
    scale: one 8-bit luma code of the input is 1 / 219 of the scale and leaves as four; the arithmetic predicts a quarter of that at 10 bits."""
    t, A = 0.25, 0.95
    g = np.linspace(0.6, 0.9, 512)
    # 8 bits: bytes in, bytes out (tensor2im's truncation, then the integer conversion)
    rgb8 = np.repeat(np.rint(g * 255).astype(np.uint8)[None, :, None], 3, axis=2)                       # (1, 512, 3)
    seen8 = ref8.yuv_to_rgb(ref8.rgb_to_yuv(rgb8, "444", "bt601", False), 1, 512, "444", "bt601", False).astype(np.float64) / 255
    out8 = (np.clip((seen8 - A) / t + A, 0, 1) * 255).astype(np.uint8)
    y8 = ref8.rgb_to_yuv(out8, "444", "bt601", False)[:512].astype(np.int64)
    # 10 bits: floats in [-1, 1] both ways
    x = np.repeat((2 * g - 1).astype(np.float32)[None, None, :], 3, axis=0)                             # (3, 1, 512)
    seen10 = (ref.yuv_to_rgb(ref.rgb_to_yuv(x, "444", 10, "bt601", False), 1, 512, "444", 10, "bt601", False).astype(np.float64) + 1) / 2
    out10 = (2 * np.clip((seen10 - A) / t + A, 0, 1) - 1).astype(np.float32)
    y10 = ref.samples(ref.rgb_to_yuv(out10, "444", 10, "bt601", False))[:512].astype(np.int64)
    step8, step10 = int(np.abs(np.diff(y8)).max()) / 255.0, int(np.abs(np.diff(y10)).max()) / 1023.0
    print("largest step: 8 bits %d codes = %.5f of full scale, 10 bits %d codes = %.5f; ratio %.3f"
          % (np.abs(np.diff(y8)).max(), step8, np.abs(np.diff(y10)).max(), step10, step10 / step8))
    assert y8.max() > y8.min() and y10.max() > y10.min()
    assert step10 <= 0.5 * step8
