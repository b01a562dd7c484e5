"""Scores against a ground-truth stream, host side (no GPU): the numpy restatement tests/planes_ref.py against a plain loop, the figures
gtscore.py forms from the device's words, the csv and the summary line, the refusals of dehaze_video.py --eval_gt, and the ledger of
include/cfen_planes.h."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import cabi_ledger
import planes_ref as ref
import yuv_ref
import yuv16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = {"420jpeg": (22, 23), "420mpeg2": (21, 22), "422": (12, 23), "444": (12, 13), "mono": (11, 12)}      # every plane holds a window


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("chroma", ref.CHROMAS)
def test_the_vectorised_words_are_the_plain_loop(chroma, depth):
    H, W = SMALL[chroma]
    a, b = ref.pair(H, W, chroma, depth, 3, seed=7 + depth)
    assert a.shape == (3, ref.frame_bytes(H, W, chroma, depth)) and a.dtype == np.uint8
    for prev, lo in ((None, 0), ((a[0], b[0]), 1)):
        sse, dt, ssim, count = ref.words(a[lo:], b[lo:], H, W, chroma, depth, prev)
        sse_l, dt_l, ssim_l, count_l = ref.words_loops(a[lo:], b[lo:], H, W, chroma, depth, prev)
        assert sse.tolist() == sse_l and dt.tolist() == dt_l and count.tolist() == count_l
        nplanes = 1 if chroma == "mono" else 3
        assert (count[:, :nplanes] > 0).all() and not count[:, nplanes:].any() and (sse[:, :nplanes] > 0).all()
        assert (dt[0] == 0).all() == (prev is None) and (dt[1:, :nplanes] > 0).all()
        for k in range(len(ssim_l)):
            for p in range(3):
                if p < nplanes:
                    assert abs(ssim[k, p] - ssim_l[k][p]) <= 1e-12 and 0.0 < ssim[k, p] < 1.0
                else:
                    assert math.isnan(ssim[k, p]) and math.isnan(ssim_l[k][p])
    # a batch is its frames chained through prev
    whole = ref.words(a, b, H, W, chroma, depth)
    for k in range(3):
        one = ref.words(a[k:k + 1], b[k:k + 1], H, W, chroma, depth, (a[k - 1], b[k - 1]) if k else None)
        assert all(np.array_equal(w[k], o[0], equal_nan=True) for w, o in zip(whole, one))


def test_the_fp32_evaluation_is_close_to_float64_and_no_closer():
    """the unit of the device test's bar at deep depths: the same definition in fp32 numpy lies a rounding distance from float64, not on it"""
    a, b = ref.pair(17, 33, "444", 12, 2, seed=3)
    w64, w32 = ref.words(a, b, 17, 33, "444", 12)[2], ref.words(a, b, 17, 33, "444", 12, dtype=np.float32)[2]
    d = np.abs(w64 - w32).max()
    assert 0.0 < d < 1e-5


def test_identical_frames():
    from cfen_vit_dehazing_amd import gtscore
    a, b = ref.pair(22, 23, "420jpeg", 10, 2, seed=5, kind="equal")
    assert np.array_equal(a, b)
    sse, dt, ssim, count = ref.words(a, b, 22, 23, "420jpeg", 10)
    assert not sse.any() and not dt.any() and (ssim == 1.0).all()
    rows = [gtscore.row_from_words(sse[k], dt[k], ssim[k], count[k], 10, k > 0) for k in range(2)]
    assert all(p == float("inf") for r in rows for p in r["psnr"] + [r["psnr_avg"]]) and rows[1]["dt_y"] == 0.0 and rows[0]["dt_y"] is None


def test_the_temporal_error():
    """0 when out - gt is the same in both frames; a hand-computed value on a 3 x 3 mono example"""
    rs = np.random.RandomState(1)
    gt0, gt1 = rs.randint(20, 200, (2, 9))
    offset = rs.randint(-20, 20, 9)
    frames = lambda *v: np.stack([x.astype(np.uint8) for x in v])
    sse, dt, ssim, count = ref.words(frames(gt0 + offset, gt1 + offset), frames(gt0, gt1), 3, 3, "mono", 8)
    assert dt.tolist() == [[0, 0, 0], [0, 0, 0]] and sse[0, 0] == sse[1, 0] == int((offset * offset).sum()) > 0
    out0 = np.array([10, 10, 10, 20, 20, 20, 30, 30, 30])
    out1 = np.array([12, 10, 7, 20, 25, 20, 30, 30, 31])          # the output changes by 2, 0, -3, 0, 5, 0, 0, 0, 1
    g0 = np.array([50, 50, 50, 50, 50, 50, 50, 50, 50])
    g1 = np.array([51, 50, 50, 50, 49, 50, 50, 50, 51])           # the ground truth by 1, 0, 0, 0, -1, 0, 0, 0, 1
    sse, dt, ssim, count = ref.words(frames(out0, out1), frames(g0, g1), 3, 3, "mono", 8)
    assert dt[:, 0].tolist() == [0, 1 + 0 + 3 + 0 + 6 + 0 + 0 + 0 + 0] and count[:, 0].tolist() == [9, 9]
    assert np.isnan(ssim).all()                                   # 3 x 3 holds no window
    assert ref.words(frames(out1), frames(g1), 3, 3, "mono", 8, prev=(out0.astype(np.uint8), g0.astype(np.uint8)))[1][0, 0] == 10


def test_a_sample_above_top_is_clamped():
    top = 1023
    a = ref.payload([np.array([[1023, 5000, 65535], [0, 1, 1024]])], 10)[None]
    b = ref.payload([np.array([[1023, 1023, 1023], [0, 1, 1023]])], 10)[None]
    assert a.dtype == np.uint8 and a.shape == (1, 12) and a[0, 2:4].tolist() == [5000 & 255, 5000 >> 8]
    sse, dt, ssim, count = ref.words(a, b, 2, 3, "mono", 10)
    assert sse[0, 0] == 0 and count[0, 0] == 6
    b0 = ref.payload([np.zeros((2, 3), dtype=np.int64)], 10)[None]
    assert ref.words(a, b0, 2, 3, "mono", 10)[0][0, 0] == 4 * top * top + 1
    a16, b16 = ref.pair(11, 12, "mono", 16, 1, seed=1, kind="extremes")
    assert ref.words(a16, b16, 11, 12, "mono", 16)[0][0, 0] == 65535 ** 2 * 132


def test_a_plane_under_eleven_wide_has_no_ssim_but_its_integers():
    H, W = 20, 22                                                 # C420mpeg2: chroma 10 x 11
    a, b = ref.pair(H, W, "420mpeg2", 8, 2, seed=9)
    sse, dt, ssim, count = ref.words(a, b, H, W, "420mpeg2", 8)
    assert count.tolist() == [[440, 110, 110]] * 2 and not np.isnan(ssim[:, 0]).any() and np.isnan(ssim[:, 1:]).all()
    assert (sse > 0).all() and (dt[1] > 0).all()


# ---- gtscore: the figures, the csv, the summary ------------------------------------------------------------------------------------------------------
def test_psnr():
    from cfen_vit_dehazing_amd import gtscore
    assert gtscore.psnr(0, 100, 8) == float("inf") and math.isnan(gtscore.psnr(0, 0, 8))
    assert gtscore.psnr(100 * 255 * 255, 100, 8) == 0.0
    assert abs(gtscore.psnr(400, 100, 8) - 10 * math.log10(255.0 ** 2 / 4.0)) < 1e-12
    assert abs(gtscore.psnr(400, 100, 10) - 10 * math.log10(1023.0 ** 2 / 4.0)) < 1e-12
    assert abs(gtscore.psnr(65535 ** 2 * (1 << 31), 1 << 31, 16)) < 1e-12


def test_csv_and_summary_formats():
    from cfen_vit_dehazing_amd import gtscore
    assert gtscore.CSV_HEADER == "frame,psnr_y,psnr_cb,psnr_cr,psnr_avg,ssim_y,ssim_cb,ssim_cr,dt_y,sse_y,sse_cb,sse_cr,dtsum_y,n_y,n_c"
    nan = float("nan")
    rows = [gtscore.row_from_words([40000, 2500, 10000], [0, 0, 0], [0.9, 0.95, nan], [10000, 2500, 2500], 8, False),
            gtscore.row_from_words([0, 0, 0], [0, 0, 0], [1.0, 1.0, nan], [10000, 2500, 2500], 8, True),            # an identical frame
            gtscore.row_from_words([10000, 0, 2500], [5000, 7, 7], [0.8, 1.0, nan], [10000, 2500, 2500], 8, True)]
    p = lambda sse, n: "%.6f" % (10 * math.log10(255.0 ** 2 * n / sse))
    text = gtscore.format_csv([("frame_%06d" % k, r) for k, r in enumerate(rows)])
    assert text == (gtscore.CSV_HEADER + "\n"
                    "frame_000000,%s,%s,%s,%s,0.900000000,0.950000000,nan,,40000,2500,10000,0,10000,2500\n"
                    "frame_000001,inf,inf,inf,inf,1.000000000,1.000000000,nan,0.000000,0,0,0,0,10000,2500\n"
                    "frame_000002,%s,inf,%s,%s,0.800000000,1.000000000,nan,0.500000,10000,0,2500,5000,10000,2500\n"
                    % (p(40000, 10000), p(2500, 2500), p(10000, 2500), p(52500, 15000), p(10000, 10000), p(2500, 2500), p(12500, 15000)))
    # pooled from the summed integers: the identical frame's inf does not reach the PSNR, and the first frame is no part of the temporal mean
    assert gtscore.summary_line(rows) == ("gt: 3 frames, PSNR-Y %.3f, mean SSIM-Y 0.900000, PSNR avg %.3f, mean temporal error 0.2500 levels"
                                          % (10 * math.log10(255.0 ** 2 * 30000 / 50000), 10 * math.log10(255.0 ** 2 * 45000 / 65000)))
    assert gtscore.summary_line(rows[1:2]) == "gt: 1 frames, PSNR-Y inf, mean SSIM-Y 1.000000, PSNR avg inf, mean temporal error 0.0000 levels"
    assert gtscore.summary_line(rows[:1]) .endswith("mean temporal error nan levels")
    assert gtscore.summary_line([]) == "gt: 0 frames, PSNR-Y nan, mean SSIM-Y nan, PSNR avg nan, mean temporal error nan levels"
    assert gtscore.format_csv([]) == gtscore.CSV_HEADER + "\n"
    mono = gtscore.row_from_words([400, 0, 0], [0, 0, 0], [0.5, nan, nan], [100, 0, 0], 10, False)
    assert gtscore.format_csv([("f", mono)]).splitlines()[1] == "f,%.6f,nan,nan,%.6f,0.500000000,nan,nan,,400,0,0,0,100,0" % (
        (10 * math.log10(1023.0 ** 2 / 4),) * 2)


# ---- dehaze_video.py --eval_gt: the flags and every refusal ------------------------------------------------------------------------------------------
def _y4m(path, W, H, chroma="420jpeg", depth=8, frames=1, tags=("F25:1", "Ip", "A1:1")):
    if depth == 8:
        data = yuv_ref.y4m_bytes([np.zeros(yuv_ref.frame_bytes(H, W, chroma), np.uint8)] * frames, W, H, chroma, header=yuv_ref.y4m_header(W, H, chroma, tags=tags))
    else:
        data = yuv16_ref.y4m_bytes([np.zeros(yuv16_ref.frame_bytes(H, W, chroma), np.uint8)] * frames, W, H, chroma, depth,
                                   header=yuv16_ref.y4m_header(W, H, chroma, depth, tags=tags))
    path.write_bytes(data)
    return str(path)


def _parse(tmp_path, *extra, src="clip.y4m", out=None):
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    return VideoOptions().parse(["--in", src, "--out", out or str(tmp_path / "out.y4m"), "--name", "video", "--gpu_ids", "-1",
                                 "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_eval_gt_flags_and_refusals(tmp_path, capsys):
    for args in ((), ("--eval_flicker",), ("--eval_noref",)):
        opt = _parse(tmp_path, *args)
        text = capsys.readouterr().out
        recorded = open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
        for t in (text, recorded):                                # a run without the flag prints and records what it always did
            assert not any(l.startswith(("eval_gt", "gt_csv")) for l in t.splitlines()) and "video_matrix: auto" in t
        assert not opt.eval_gt and not opt.gt_csv
    src = _y4m(tmp_path / "in.y4m", 64, 48, "420mpeg2", frames=2)
    gt = _y4m(tmp_path / "gt.y4m", 64, 48, "420mpeg2", frames=2)
    opt = _parse(tmp_path, "--eval_gt", gt, src=src)
    assert opt.eval_gt == gt and opt.gt_csv == str(tmp_path / "gt.csv")
    text = capsys.readouterr().out
    assert "eval_gt: %s" % gt in text and "eval_gt: %s" % gt in open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
    assert _parse(tmp_path, "--eval_gt", gt, "--gt_csv", "x.csv", src=src, out="-").gt_csv == "x.csv"
    assert _parse(tmp_path, "--eval_gt", gt, src="-").eval_gt == gt          # a pipe: video.run compares the headers once it has read the input's
    capsys.readouterr()

    def refused(*args, **kw):
        with pytest.raises(ValueError) as e:
            _parse(tmp_path, *args, **kw)
        assert not (tmp_path / "out.y4m").exists()
        return str(e.value)

    assert "--eval_gt" in refused("--gt_csv", "x.csv", src=src)                                  # --gt_csv alone
    assert "--gt_csv PATH" in refused("--eval_gt", gt, src=src, out="-")                         # --out - without --gt_csv
    assert "- (stdin) is refused" in refused("--eval_gt", "-", src=src)
    assert "--eval_gt" in refused("--eval_gt", str(tmp_path / "none.y4m"), src=src)              # no such file
    (tmp_path / "text.y4m").write_bytes(b"not a stream\n")
    assert "not a YUV4MPEG2 stream" in refused("--eval_gt", str(tmp_path / "text.y4m"), src=src)
    # mismatched size, tag, depth and interlacing: both values are named
    msg = refused("--eval_gt", _y4m(tmp_path / "w.y4m", 66, 48, "420mpeg2"), src=src)
    assert "width is 66 but the input's is 64" in msg
    msg = refused("--eval_gt", _y4m(tmp_path / "h.y4m", 64, 50, "420mpeg2"), src=src)
    assert "height is 50 but the input's is 48" in msg
    msg = refused("--eval_gt", _y4m(tmp_path / "c.y4m", 64, 48, "420jpeg"), src=src)
    assert "C tag is C420jpeg but the input's is C420mpeg2" in msg
    msg = refused("--eval_gt", _y4m(tmp_path / "i.y4m", 64, 48, "420mpeg2", tags=("F25:1", "A1:1")), src=src)
    assert "interlacing is I? but the input's is Ip" in msg
    assert "interlaced stream" in refused("--eval_gt", _y4m(tmp_path / "it.y4m", 64, 48, "420mpeg2", tags=("F25:1", "It", "A1:1")), src=src)
    deep = _y4m(tmp_path / "d.y4m", 64, 48, "420mpeg2", depth=10)
    assert "high bit depth" in refused("--eval_gt", deep, src=src)                               # without --video_depth auto nothing deep is read
    msg = refused("--eval_gt", deep, "--video_depth", "auto", src=src)
    assert "C tag is C420p10 but the input's is C420mpeg2" in msg
    msg = refused("--eval_gt", _y4m(tmp_path / "d12.y4m", 64, 48, "420mpeg2", depth=12), "--video_depth", "auto", src=deep)
    assert "C tag is C420p12 but the input's is C420p10" in msg
    assert _parse(tmp_path, "--eval_gt", deep, "--video_depth", "auto", src=deep).eval_gt == deep
    # `C420` and no C tag at all are C420jpeg: the same format under another spelling is taken
    plain = tmp_path / "plain.y4m"
    plain.write_bytes(b"YUV4MPEG2 W64 H48 F25:1 Ip A1:1\n")
    assert _parse(tmp_path, "--eval_gt", _y4m(tmp_path / "j.y4m", 64, 48, "420jpeg"), src=str(plain)).eval_gt


def test_the_headers_are_compared_again_where_a_pipe_is_read():
    from cfen_vit_dehazing_amd import video
    a = video.parse_header(b"YUV4MPEG2 W64 H48 F25:1 Ip A1:1 C444p12\n", 16)
    video.check_gt_header(a, dict(a))
    for line, what in ((b"YUV4MPEG2 W64 H48 Ip C444p10\n", "C tag is C444p10 but the input's is C444p12"),
                       (b"YUV4MPEG2 W32 H48 Ip C444p12\n", "width is 32 but the input's is 64")):
        with pytest.raises(video.Y4MError, match=re.escape(what)):
            video.check_gt_header(a, video.parse_header(line, 16), "clear.y4m")


def test_test_py_does_not_get_the_flag():
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    o = TestOptions()
    o.initialize()
    assert "eval_gt" not in o.parser.format_help()
    from cfen_vit_dehazing_amd import video
    assert video.DEEP_REFUSED == ("fit", "temporal", "eval_noref", "eval_flicker")


# ---- the new header's ledger ------------------------------------------------------------------------------------------------------------------------
def test_planes_header_is_exported_bound_and_apart_from_the_older_tables():
    fns = {"cfen_plane_metrics_bytes": 4, "cfen_plane_metrics": 14}
    cabi_ledger.check_header_bound("cfen_planes.h", fns, word="plane_metrics")
    cabi_ledger.check_guard_band_test_calls("test_hip_plane_metrics.py", "test_guard_bands_plane_metrics", ["cfen_plane_metrics"])
    from cfen_vit_dehazing_amd import _lib
    assert len(_lib.SIGNATURES) == 68 and _lib.load().cfen_abi_version() == 1


def test_the_definition_stands_in_the_header():
    text = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "cfen_planes.h")).read()).split())
    for phrase in ("word 0, uint64: SSE = sum (a - b)^2 over the plane. Exact integer.",
                   "word 1, uint64: DT = sum |(a - a_prev) - (b - b_prev)| over the plane", "0 when there is no previous frame.",
                   "x = (float)v / (float)top, one IEEE division", "11 x 11 Gaussian window, sigma 1.5, valid convolution, C1 = 0.01^2, C2 = 0.03^2",
                   "fp32 map arithmetic, fixed-order fp64 sums", "A plane with h < 11 or w < 11 gets NaN here. Its integers are still written.",
                   "word 3, uint64: the plane's sample count h w, or 0 for a plane the format does not have",
                   "A stored value above top reads as top.", "Two little-endian bytes at depths 9 .. 16.", "No global atomics"):
        assert phrase in text, phrase


def test_the_scratch_size_and_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    tiles = lambda h, w: max(1, -(-(h - 10) // 24)) * max(1, -(-(w - 10) // 64))
    for B, H, W, chroma in ((1, 11, 11, "mono"), (3, 22, 23, "420jpeg"), (2, 130, 259, "420jpeg"), (1, 2160, 3840, "420mpeg2"), (1, 3, 3, "444"),
                            (2, 35, 75, "422"), (1, 32768, 65536, "mono")):
        shapes = ref.plane_shapes(H, W, chroma)
        assert lib.cfen_plane_metrics_bytes(B, H, W, yuv_ref.CHROMAS.index(chroma)) == 24 * B * sum(tiles(h, w) for h, w in shapes), (B, H, W, chroma)
    for bad in ((0, 20, 20, 0), (65536, 20, 20, 0), (1, 0, 20, 0), (1, 20, 65537, 0), (1, 20, 20, 5), (1, 20, 20, -1), (1, 65536, 32769, 4)):
        assert lib.cfen_plane_metrics_bytes(*bad) == 0, bad
    a, b, qa, qb, sc, out, z = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5, 6, 0))      # never dereferenced
    refused, off = functools.partial(cabi_ledger.refused, lib, "plane_metrics"), cabi_ledger.off
    nb = 20 * 20 + 2 * 10 * 10
    good = [a, nb, b, nb, qa, qb, 1, 20, 20, 0, 8, sc, out, z]
    for i in (0, 2, 11, 12):
        args = list(good)
        args[i] = z
        refused(b"null pointer", *args)
    for i in (4, 5):
        args = list(good)
        args[i] = z
        refused(b"both be NULL or both be set", *args)

    def with_(**kw):
        names = ("a", "stride_a", "b", "stride_b", "a_prev", "b_prev", "B", "H", "W", "chroma", "depth", "scratch", "out", "stream")
        return [kw.get(n, v) for n, v in zip(names, good)]
    refused(b"B = 0", *with_(B=0))
    refused(b"B = 65536", *with_(B=65536))
    refused(b"H = 0", *with_(H=0))
    refused(b"W = 65537", *with_(W=65537, stride_a=1 << 40, stride_b=1 << 40))
    refused(b"over 2^31", *with_(H=65536, W=32769, chroma=4, stride_a=1 << 40, stride_b=1 << 40))
    for c in (-1, 5):
        refused(b"unknown chroma format %d" % c, *with_(chroma=c))
    for d in (7, 17, 0):
        refused(b"depth = %d" % d, *with_(depth=d, stride_a=2 * nb, stride_b=2 * nb))
    refused(b"below the frame size 600", *with_(stride_a=nb - 1))
    refused(b"below the frame size 600", *with_(stride_b=nb - 1))
    refused(b"below the frame size 1200", *with_(depth=10))
    deep = dict(depth=10, stride_a=2 * nb, stride_b=2 * nb)
    for odd in (dict(a=off(a, 1)), dict(b=off(b, 1)), dict(a_prev=off(qa, 1)), dict(b_prev=off(qb, 3)), dict(stride_a=2 * nb + 1), dict(stride_b=2 * nb + 3)):
        refused(b"an odd pointer or stride", *with_(**dict(deep, **odd)))
    for bad in (dict(out=off(out, 4)), dict(scratch=off(sc, 4)), dict(out=off(out, 1)), dict(scratch=off(sc, 2))):
        refused(b"8-byte aligned", *with_(**bad))
