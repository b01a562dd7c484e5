"""Host side of the YCbCr <-> RGB extension: the integer tables (cfen_vit_dehazing_amd/yuv.py) against their known answers and the float64
formulas, the chroma resampling of the restatement (tests/yuv_ref.py), the y4m reader and writer (cfen_vit_dehazing_amd/video.py), and the
ledger of include/cfen_yuv.h.

Bars of the exhaustive runs over all 2^24 triples:
  integer forward / inverse against float64   <= 1.  From the arithmetic: coefficient rounding contributes at most 3 * 255 * 2^-15 = 0.024, the
                                              final rounding 0.5 (0.524 in all; the row-sum repair moves one luma or chroma coefficient by at
                                              most one more unit: + 255 * 2^-14 = 0.016).  Measured 0.51.
  RGB -> YCbCr -> RGB at 4:4:4                <= 2 levels limited range, <= 1 full range
  greys                                       <= 1 limited, 0 full"""
import io
import os
import re
import threading

import numpy as np
import pytest

from cfen_vit_dehazing_amd import video, yuv
import cabi_ledger
import yuv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
SIZES = [(1, 1), (3, 5), (8, 8)]


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", COMBOS)
def test_tables_are_the_known_answers(matrix, full):
    fwd, inv, oy = yuv.tables(matrix, full)
    wf, wi, woy = ref.table(matrix, full)
    assert fwd.dtype == np.int32 and inv.dtype == np.int32 and fwd.shape == (3, 3) and inv.shape == (3, 3)
    assert fwd.tolist() == wf.tolist() and inv.tolist() == wi.tolist() and oy == woy == (0 if full else 16)
    assert fwd[0].sum() == round((255 if full else 219) / 255 * 2 ** 14) and fwd[1].sum() == 0 and fwd[2].sum() == 0
    with pytest.raises(ValueError, match="matrix"):
        yuv.tables("bt2020", full)


@pytest.mark.parametrize("matrix,full", COMBOS)
def test_exhaustive_bounds_over_all_2_24_triples(matrix, full):
    fwd, inv, oy = (np.asarray(t).astype(np.int64) if k < 2 else t for k, t in enumerate(yuv.tables(matrix, full)))
    ff, fi, _ = yuv.float_matrices(matrix, full)
    off = np.array([oy, 128.0, 128.0])
    g, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    plane = np.stack([np.zeros_like(g), g, b], axis=-1)                          # (256, 256, 3), the first component is set per step
    worst_f = worst_i = 0.0
    worst_rt = worst_grey = 0
    for r in range(256):
        plane[..., 0] = r
        ycc = ref.forward_pixels(plane, fwd, oy)
        want = np.clip(plane @ ff.T + off, 0, 255)
        worst_f = max(worst_f, float(np.abs(ycc - want).max()))
        back = ref.inverse_pixels(ycc, inv, oy)                                  # the round trip of the RGB triples (r, g, b)
        worst_rt = max(worst_rt, int(np.abs(back - plane).max()))
        worst_grey = max(worst_grey, int(np.abs(back[r, r] - r).max()))
        assert ycc[r, r, 1] == 128 and ycc[r, r, 2] == 128                       # R = G = B gives Cb = Cr = 128 exactly
        rgb = ref.inverse_pixels(plane, inv, oy)                                 # the same triples read as (Y, Cb, Cr): out of gamut included
        want = np.clip((plane - off) @ fi.T, 0, 255)
        worst_i = max(worst_i, float(np.abs(rgb - want).max()))
    print("%s %s: forward %.4f, inverse %.4f, round trip %d, greys %d" % (matrix, "full" if full else "limited", worst_f, worst_i, worst_rt, worst_grey))
    assert worst_f <= 1 and worst_i <= 1
    assert worst_rt <= (1 if full else 2)
    assert worst_grey <= (0 if full else 1)


# ---- chroma resampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_constant_chroma_survives_up_and_down_exactly(chroma):
    if chroma == "mono":
        assert ref.chroma_shape(3, 5, chroma) == (0, 0) and ref.frame_bytes(3, 5, chroma) == 15
        return
    for H, W in SIZES:
        hc, wc = ref.chroma_shape(H, W, chroma)
        assert (hc, wc) == yuv.chroma_shape(H, W, chroma) and ref.frame_bytes(H, W, chroma) == yuv.frame_bytes(H, W, chroma)
        for v in (0, 1, 77, 128, 254, 255):
            up = ref.upsample(np.full((hc, wc), v), H, W, chroma)
            assert up.shape == (H, W) and (up == v).all()
            down = ref.downsample(np.full((H, W), v), chroma)
            assert down.shape == (hc, wc) and (down == v).all()


@pytest.mark.parametrize("chroma", ref.CHROMAS)
@pytest.mark.parametrize("matrix,full", [("bt601", False), ("bt709", True)])
def test_a_grey_image_comes_back(chroma, matrix, full):
    rs = np.random.RandomState(3)
    for H, W in SIZES + [(5, 7)]:
        grey = np.repeat(rs.randint(0, 256, (H, W, 1)), 3, axis=2).astype(np.uint8)
        frame = ref.rgb_to_yuv(grey, chroma, matrix, full)
        assert frame.size == ref.frame_bytes(H, W, chroma)
        if chroma != "mono":
            assert (frame[H * W:] == 128).all()
        back = ref.yuv_to_rgb(frame, H, W, chroma, matrix, full)
        assert np.abs(back.astype(int) - grey).max() <= (0 if full else 1)


@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_upsampling_weights_sum_to_16(chroma):
    assert (ref.upsample_weights(5, 7, chroma) == 16).all() and ref.upsample_weights(5, 7, chroma).shape == (5, 7)


@pytest.mark.parametrize("chroma", [c for c in ref.CHROMAS if c != "mono"])
def test_loops_agree_with_the_vectorised_restatement(chroma):
    rs = np.random.RandomState(5)
    for H, W in SIZES + [(5, 7), (6, 9)]:
        hc, wc = ref.chroma_shape(H, W, chroma)
        c = rs.randint(0, 256, (hc, wc))
        assert np.array_equal(ref.upsample(c, H, W, chroma), ref.upsample_loops(c, H, W, chroma))
        d = rs.randint(0, 256, (H, W))
        assert np.array_equal(ref.downsample(d, chroma), ref.downsample_loops(d, chroma))
        frame = rs.randint(0, 256, ref.frame_bytes(H, W, chroma)).astype(np.uint8)
        assert np.array_equal(ref.yuv_to_rgb(frame, H, W, chroma), ref.yuv_to_rgb(frame, H, W, chroma, up=ref.upsample_loops))
        rgb = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        assert np.array_equal(ref.rgb_to_yuv(rgb, chroma), ref.rgb_to_yuv(rgb, chroma, down=ref.downsample_loops))


# ---- reader and writer -----------------------------------------------------------------------------------------------------------------
def _frames(n, H, W, chroma, seed=0):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, ref.frame_bytes(H, W, chroma)).astype(np.uint8) for _ in range(n)]


@pytest.mark.parametrize("header,chroma,crange", [
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420jpeg\n", "420jpeg", None),
    (b"YUV4MPEG2 W6 H4 F30000:1001 Ip A0:0 C420mpeg2 XYSCSS=420MPEG2\n", "420mpeg2", None),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C422\n", "422", None),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C444 XCOLORRANGE=FULL\n", "444", "full"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 Cmono XCOLORRANGE=LIMITED\n", "mono", "limited"),
    (b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420\n", "420jpeg", None),
    (b"YUV4MPEG2 W6 H4 F25:1\n", "420jpeg", None),                      # no C and no I tag: mjpegtools' defaults
    (b"YUV4MPEG2 H4 W6 I? F25:1\n", "420jpeg", None),
])
def test_reader_takes_every_accepted_header_and_the_writer_repeats_it(header, chroma, crange, tmp_path):
    frames = _frames(3, 4, 6, chroma)
    data = ref.y4m_bytes(frames, 6, 4, chroma, header=header)
    r = video.Y4MReader(io.BytesIO(data))
    assert (r.width, r.height, r.chroma, r.color_range, r.header) == (6, 4, chroma, crange, header)
    assert r.frame_bytes == ref.frame_bytes(4, 6, chroma) and r.check_whole_file() == 3
    out = io.BytesIO()
    w = video.Y4MWriter(out, r.header)
    n = 0
    while True:
        f = r.read_frame()
        if f is None:
            break
        assert f == frames[n].tobytes()
        w.write_frame(f)
        n += 1
    w.close()
    assert n == 3 and r.frames_read == 3 and w.frames_written == 3
    assert out.getvalue() == data                                      # header byte for byte, plain FRAME lines
    # through files, and FRAME lines with parameters
    path = tmp_path / "a.y4m"
    path.write_bytes(ref.y4m_bytes(frames, 6, 4, chroma, header=header, frame_line=b"FRAME Ip\n"))
    r = video.Y4MReader(str(path))
    assert r.check_whole_file() == 3
    w = video.Y4MWriter(str(tmp_path / "b.y4m"), r.header)
    buf = bytearray(r.frame_bytes)
    while r.read_frame_into(buf):
        w.write_frame(buf)
    w.close()
    r.close()
    assert (tmp_path / "b.y4m").read_bytes() == data


def test_a_stream_without_frames_still_gets_its_header():
    out = io.BytesIO()
    r = video.Y4MReader(io.BytesIO(b"YUV4MPEG2 W6 H4\n"))
    assert r.read_frame() is None and r.check_whole_file() == 0
    video.Y4MWriter(out, r.header).close()
    assert out.getvalue() == b"YUV4MPEG2 W6 H4\n"


def test_a_pipe_that_delivers_a_few_bytes_at_a_time():
    frames = _frames(3, 5, 7, "420jpeg", seed=1)
    data = ref.y4m_bytes(frames, 7, 5)
    rfd, wfd = os.pipe()

    def feed():
        rs, pos = np.random.RandomState(2), 0
        with os.fdopen(wfd, "wb", buffering=0) as f:
            while pos < len(data):
                n = int(rs.randint(1, 8))
                f.write(data[pos:pos + n])
                pos += n
    t = threading.Thread(target=feed)
    t.start()
    with os.fdopen(rfd, "rb") as f:
        r = video.Y4MReader(f)
        assert r.check_whole_file() is None                            # a pipe cannot be walked ahead of time
        got = []
        while True:
            x = r.read_frame()
            if x is None:
                break
            got.append(x)
    t.join()
    assert got == [f.tobytes() for f in frames]


@pytest.mark.parametrize("header,names", [
    (b"YUV4MPEG2 W6 H4 F25:1 Ip C420p10\n", "C420p10"), (b"YUV4MPEG2 W6 H4 C444p12\n", "C444p12"), (b"YUV4MPEG2 W6 H4 C422p16\n", "C422p16"),
    (b"YUV4MPEG2 W6 H4 C420p9\n", "C420p9"), (b"YUV4MPEG2 W6 H4 Cmono16\n", "Cmono16"),
    (b"YUV4MPEG2 W6 H4 C420paldv\n", "C420paldv"), (b"YUV4MPEG2 W6 H4 It\n", "It"), (b"YUV4MPEG2 W6 H4 Ib\n", "Ib"), (b"YUV4MPEG2 W6 H4 Im\n", "Im"),
    (b"YUV4MPEG2 W6 H4 XCOLORRANGE=WIDE\n", "XCOLORRANGE=WIDE"), (b"YUV4MPEG2 W0 H4\n", "W0"), (b"YUV4MPEG2 W6\n", "no H tag"),
    (b"RIFF....AVI \n", "YUV4MPEG2"), (b"YUV4MPEG2 W6 H4", "ends inside"),
])
def test_reader_refuses_what_it_cannot_dehaze_and_names_it(header, names):
    with pytest.raises(video.Y4MError, match=re.escape(names)):
        video.Y4MReader(io.BytesIO(header + (b"FRAME\n" + bytes(36) if header.endswith(b"\n") else b"")))


def test_a_frame_cut_short_is_named_by_its_index():
    frames = _frames(3, 4, 6, "420jpeg")
    data = ref.y4m_bytes(frames, 6, 4)
    for cut, where in ((5, "frame 2"), (len(frames[0]) + 6 + 3, "frame 1"), (len(frames[0]) + 3, "frame 2")):
        r = video.Y4MReader(io.BytesIO(data[:-cut]))
        with pytest.raises(video.Y4MError, match=where + " is cut short"):
            r.check_whole_file()                                       # a file: before anything is read
        with pytest.raises(video.Y4MError, match=where + " is cut short"):
            while r.read_frame() is not None:                          # a pipe: when it is reached
                pass
    r = video.Y4MReader(io.BytesIO(data[:-len(frames[0]) - 2]))      # inside a FRAME line
    with pytest.raises(video.Y4MError, match="frame 2 is cut short"):
        while r.read_frame() is not None:
            pass
    r = video.Y4MReader(io.BytesIO(data.replace(b"FRAME\n", b"FRAMX\n")))
    with pytest.raises(video.Y4MError, match="frame 0: expected a FRAME line"):
        r.read_frame()


# ---- the ring between the reader, the caller and the writer ------------------------------------------------------------------------------
def _pump(data, target, batch, k, process=None, limit=20.0):
    """video.pump over the stream `data` into `target` on a thread of its own: (frames or None, the exception or None); fails if it does not end"""
    reader = video.Y4MReader(io.BytesIO(data))
    writer = video.Y4MWriter(target, reader.header)
    slots = [video.Slot(np.zeros((batch, reader.frame_bytes), np.uint8), np.zeros((batch, reader.frame_bytes), np.uint8)) for _ in range(k)]

    def invert(s):
        s.rows_out[:s.n] = 255 - s.rows_in[:s.n]
    result = []

    def body():
        try:
            result.append((video.pump(reader, writer, batch, slots, process or invert), None))
        except BaseException as e:
            result.append((None, e))
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(limit)
    assert not t.is_alive(), "pump did not end within %g s: the ring is stuck" % limit
    return result[0]


class _FailingTarget(io.BytesIO):
    """a file whose write raises once `budget` bytes have been taken: a pipe whose reader has gone, a full disk"""

    def __init__(self, budget, error):
        super().__init__()
        self.budget, self.error = budget, error

    def write(self, b):
        if self.tell() + len(b) > self.budget:
            raise self.error
        return super().write(b)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_pump_keeps_frame_order_whatever_the_number_of_slots(k):
    frames = _frames(11, 4, 6, "420jpeg", seed=4)
    data = ref.y4m_bytes(frames, 6, 4)
    out = io.BytesIO()
    n, err = _pump(data, out, 3, k)
    assert err is None and n == 11
    assert out.getvalue() == ref.y4m_bytes([255 - f for f in frames], 6, 4)


@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("after_frames", [0, 1, 7])
def test_a_failed_write_ends_the_run_with_the_writers_exception(k, after_frames):
    frames = _frames(40, 4, 6, "420jpeg", seed=5)
    data = ref.y4m_bytes(frames, 6, 4)
    header = len(ref.y4m_header(6, 4))
    for error in (BrokenPipeError(32, "Broken pipe"), OSError(28, "No space left on device")):
        target = _FailingTarget(header + after_frames * (6 + len(frames[0])) + 3, error)
        n, err = _pump(data, target, 2, k)
        assert n is None and err is error, (k, after_frames, err)
        assert target.getvalue().startswith(ref.y4m_bytes([255 - f for f in frames[:after_frames]], 6, 4))


def test_a_failed_write_ends_the_run_while_the_reader_waits_for_its_pipe():
    """the consumer goes away while the producer is idle: the caller is waiting for frames, the reader for bytes; the run still ends"""
    frames = _frames(2, 4, 6, "420jpeg", seed=6)
    data = ref.y4m_bytes(frames, 6, 4)
    rfd, wfd = os.pipe()
    error = BrokenPipeError(32, "Broken pipe")
    with os.fdopen(rfd, "rb") as src, os.fdopen(wfd, "wb", buffering=0) as feed:
        feed.write(data)                                                # two frames arrive, then nothing: the write end stays open
        reader = video.Y4MReader(src)
        writer = video.Y4MWriter(_FailingTarget(len(reader.header) + 10, error), reader.header)
        slots = [video.Slot(np.zeros((1, reader.frame_bytes), np.uint8), np.zeros((1, reader.frame_bytes), np.uint8)) for _ in range(2)]
        result = []

        def body():
            try:
                video.pump(reader, writer, 1, slots, lambda s: None)
            except BaseException as e:
                result.append(e)
        t = threading.Thread(target=body, daemon=True)
        t.start()
        t.join(20.0)
        assert not t.is_alive() and result == [error]


@pytest.mark.parametrize("k", [1, 4])
def test_frames_read_before_a_cut_are_written_before_the_cut_is_reported(k):
    frames = _frames(9, 4, 6, "420jpeg", seed=7)
    data = ref.y4m_bytes(frames, 6, 4)
    out = io.BytesIO()
    n, err = _pump(data[:-5], out, 2, k)                                # frame 8, alone in the last batch, is cut
    assert n is None and isinstance(err, video.Y4MError) and "frame 8 is cut short" in str(err)
    assert out.getvalue() == ref.y4m_bytes([255 - f for f in frames[:8]], 6, 4)
    out = io.BytesIO()
    n, err = _pump(data[:-5 - 6 - len(frames[0])], out, 4, k)           # frame 7, the last of a batch of four, is cut: 4, 5, 6 still leave
    assert "frame 7 is cut short" in str(err) and out.getvalue() == ref.y4m_bytes([255 - f for f in frames[:7]], 6, 4)


def test_a_failure_in_process_ends_the_run_after_what_was_handed_over():
    frames = _frames(6, 4, 6, "420jpeg", seed=8)
    out = io.BytesIO()
    boom = RuntimeError("device")

    def process(s):
        if s.first >= 4:
            raise boom
        s.rows_out[:s.n] = s.rows_in[:s.n]
    n, err = _pump(ref.y4m_bytes(frames, 6, 4), out, 2, 2, process)
    assert err is boom and out.getvalue() == ref.y4m_bytes(frames[:4], 6, 4)


def test_matrix_and_range_choices():
    assert video.pick_matrix("auto", 719) == "bt601" and video.pick_matrix("auto", 720) == "bt709" and video.pick_matrix("bt601", 2160) == "bt601"
    assert video.pick_range("auto", None) == "limited" and video.pick_range("auto", "full") == "full" and video.pick_range("limited", "full") == "limited"


# ---- the header's ledger ---------------------------------------------------------------------------------------------------------------
def test_every_function_of_the_yuv_header_is_bound_and_guard_band_tested():
    from cfen_vit_dehazing_amd import _lib
    fns = {"cfen_yuv_frame_bytes": 3, "cfen_yuv_to_rgb_u8": 9, "cfen_rgb_to_yuv_u8": 9}
    cabi_ledger.check_header_bound("cfen_yuv.h", fns)
    import ctypes
    assert ctypes.sizeof(_lib.YuvTableC) == 64
    cabi_ledger.check_guard_band_test_calls("test_hip_yuv.py", "test_guard_bands_yuv", fns)
    assert yuv.CHROMA == {"420jpeg": 0, "420mpeg2": 1, "422": 2, "444": 3, "mono": 4}
    text = open(os.path.join(ROOT, "include", "cfen_yuv.h")).read()
    for name, code in yuv.CHROMA.items():
        assert re.search(r"#define CFEN_YUV_%s %d\b" % (name.upper(), code), text), name


def test_the_built_library_holds_no_fused_byte_packing():
    """hipcc's v_ashr_pk_u8_i32 packing gave wrong bytes on the device (csrc/k_yuv.hip, yv_dot): the workaround must hold with the compiler in use"""
    from cfen_vit_dehazing_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    n = build.check_no_ashr_pk_u8(_lib.LIB_PATH)
    print("v_ashr_pk_u8_i32 in the library: %s" % n)
    assert n in (0, None)
