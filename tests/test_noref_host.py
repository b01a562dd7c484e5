"""No-reference statistics (include/cfen_noref.h) on the host: the numpy restatement tests/noref_ref.py against a brute-force double loop and against
known answers, the scores of metrics.noref_from_stats, the header's ledger, the scratch size and the argument errors of the entry point, the
--eval_noref options, the csv / summary text and the float -> byte recovery of the hazy image.  No GPU."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import cabi_ledger
import noref_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,r", [((1, 1, 1), 7), ((2, 3, 5), 7), ((1, 9, 11), 0), ((1, 9, 11), 1), ((2, 12, 7), 3), ((1, 5, 40), 16), ((1, 20, 1), 2)])
def test_restatement_equals_the_brute_force_double_loop(shape, r):
    rs = np.random.RandomState(sum(shape) + r)
    hazy, out = ref._random(shape, rs)
    hazy[0, 0, 0] = 0                     # some saturated lumas on both sides
    out[0, -1, -1] = 255
    hazy[-1, -1, -1] = 255
    counts, grad, maps = ref.stats(hazy, out, r)
    bc, bg, bm = ref.brute_force(hazy, out, r)
    assert np.array_equal(counts, bc) and np.array_equal(maps, bm)
    assert np.abs(grad - bg).max() <= 1e-12 * max(1.0, np.abs(bg).max())
    assert (counts[:, :, 258] == 0).all() and (counts[:, :, :256].sum(axis=2) == shape[1] * shape[2]).all()
    if r == 0:
        assert np.array_equal(maps[0], hazy.min(axis=-1)) and np.array_equal(maps[1], out.min(axis=-1))


def test_luma_weights():
    assert ref.luma(np.array([255, 255, 255], np.uint8)) == 255 and ref.luma(np.array([0, 0, 0], np.uint8)) == 0
    assert ref.luma(np.array([255, 0, 0], np.uint8)) == (77 * 255 + 128) >> 8 == 77
    assert ref.luma(np.array([0, 255, 0], np.uint8)) == 149 and ref.luma(np.array([0, 0, 255], np.uint8)) == 29
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(ref.luma(np.stack([v, v, v], -1)), v)


def _scores(hazy, out, r=7):
    from cfen_vit_dehazing_amd import metrics
    counts, grad, _ = ref.stats(hazy, out, r)
    rows = metrics.noref_from_stats(counts, grad, hazy.shape[1], hazy.shape[2])
    want = ref.scores_from_stats(counts, grad, hazy.shape[1], hazy.shape[2])
    assert len(rows) == hazy.shape[0] and all(len(r_) == 9 and all(isinstance(v, float) for v in r_) for r_ in rows)
    got = np.array(rows)
    both = np.isnan(got) & np.isnan(want)
    assert (both | (np.abs(got - want) <= 1e-12)).all()                     # two restatements of the formulas, one in Python integers
    return [dict(zip(metrics.NOREF_COLUMNS, r_)) for r_ in rows]


@pytest.mark.parametrize("v", [0, 1, 93, 254, 255])
def test_constant_image(v):
    img = np.full((1, 20, 23, 3), v, np.uint8)
    s = _scores(img, img)[0]
    assert s["dark_in"] == s["dark_out"] == v / 255.0
    for k in ("entropy_in", "entropy_out", "contrast_in", "contrast_out", "avg_gradient_in", "avg_gradient_out", "saturated"):
        assert s[k] == 0.0 and math.copysign(1.0, s[k]) == 1.0, k          # +0.0: the csv never shows -0.000000


def test_checkerboard():
    lo, hi = 40, 200
    yy, xx = np.mgrid[0:16, 0:18]
    img = np.where(((yy + xx) & 1)[..., None] == 0, lo, hi).astype(np.uint8).repeat(3, axis=-1)[None]
    s = _scores(img, img, r=1)[0]
    assert s["entropy_in"] == 1.0                                           # two levels, half each: 1 bit
    assert abs(s["avg_gradient_in"] - (hi - lo)) <= 1e-12                   # |dx| = |dy| = hi - lo everywhere: sqrt(0.5 * 2 d^2) = d
    assert abs(s["contrast_in"] - (hi - lo) / 2 / 255.0) <= 1e-15           # two equal masses at distance d: sigma = d / 2
    assert s["dark_in"] == lo / 255.0                                       # every 3 x 3 window holds a dark square
    assert s["saturated"] == 0.0


def test_saturation_counts_only_new_pixels():
    black, white = np.zeros((1, 6, 7, 3), np.uint8), np.full((1, 6, 7, 3), 255, np.uint8)
    grey = np.full((1, 6, 7, 3), 128, np.uint8)
    assert _scores(grey, white)[0]["saturated"] == 1.0 and _scores(grey, black)[0]["saturated"] == 1.0
    assert _scores(black, white)[0]["saturated"] == 0.0                     # all-0 -> all-255: every pixel was saturated already
    counts = ref.stats(black, white, 7)[0]
    assert counts[0, 0, 257] == 42 and counts[0, 1, 257] == 0
    hazy = grey.copy()
    hazy[0, 2, 3] = 255                                                     # one pixel already saturated in the hazy image is not counted
    hazy[0, 4, 1] = 0
    s = _scores(hazy, white)[0]
    assert s["saturated"] == 40 / 42.0
    counts = ref.stats(hazy, white, 7)[0]
    assert counts[0, 0, 257] == 2 and counts[0, 1, 257] == 40
    assert _scores(grey, grey)[0]["saturated"] == 0.0


def test_gradient_is_nan_without_a_position():
    rs = np.random.RandomState(2)
    for shape in ((1, 1, 9), (1, 9, 1), (1, 1, 1)):
        hazy, out = ref._random(shape, rs)
        s = _scores(hazy, out)[0]
        assert math.isnan(s["avg_gradient_in"]) and math.isnan(s["avg_gradient_out"])
        assert ref.stats(hazy, out, 7)[1].tolist() == [[0.0, 0.0]]


def test_scattering_scene_has_more_haze_and_less_gradient_than_its_clear_image():
    """I = J t + A (1 - t): the hazy image has the larger dark channel and the smaller average gradient"""
    rs = np.random.RandomState(11)
    H, W = 96, 128
    J = rs.rand(H, W, 3) ** 2                                               # a textured scene with dark pixels in every window
    depth = np.linspace(0.2, 2.5, W)[None, :, None] * np.ones((H, 1, 1))
    t = np.exp(-0.8 * depth)
    A = 0.9
    I = J * t + A * (1 - t)
    hazy = np.round(I * 255).astype(np.uint8)[None]
    clear = np.round(J * 255).astype(np.uint8)[None]
    s = _scores(hazy, clear)[0]
    assert s["dark_in"] > s["dark_out"] + 0.2 and s["avg_gradient_in"] < 0.7 * s["avg_gradient_out"]
    assert s["contrast_in"] < s["contrast_out"]


def test_dot_footprint():
    hazy, out, r, counts, grad, maps = ref.case("dot_r16")
    y, x = ref.DOT_AT[0]
    assert (maps[0, 0] == 0).sum() == 33 * 33 and (maps[0, 0][y - 16:y + 17, x - 16:x + 17] == 0).all()
    assert (maps[0, 1] == 0).sum() == 17 * 17 and (maps[0, 1][:17, :17] == 0).all()      # clipped at the image's corner
    assert (maps[1, 0] == 7).sum() == 33 * 33 and set(np.unique(maps)) == {0, 7, 255}
    assert y < ref.TILE_H <= y + 16 and x - 16 < ref.TILE_W <= x                       # the footprint crosses a tile corner


# ---- the header's ledger ---------------------------------------------------------------------------------------------------------------------------
def test_noref_header_is_exported_bound_and_apart_from_the_frozen_abi():
    cabi_ledger.check_header_bound("cfen_noref.h", {"cfen_noref_bytes": 4, "cfen_noref_u8": 12})


def test_tile_shape_and_record_size_are_the_headers():
    from cfen_vit_dehazing_amd import metrics, ops
    text = open(os.path.join(ROOT, "include", "cfen_noref.h")).read()
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (CFEN_NOREF_[A-Z_]+) (\d+)", text)}
    assert defines == {"CFEN_NOREF_TILE_W": ops.NOREF_TILE_W, "CFEN_NOREF_TILE_H": ops.NOREF_TILE_H,
                       "CFEN_NOREF_RECORD_BYTES": ops.NOREF_RECORD_BYTES, "CFEN_NOREF_MAX_RADIUS": ops.NOREF_MAX_RADIUS}
    assert (ref.TILE_W, ref.TILE_H) == (ops.NOREF_TILE_W, ops.NOREF_TILE_H) and metrics.NOREF_MAX_RADIUS == ops.NOREF_MAX_RADIUS == 16
    assert ops.NOREF_RECORD_BYTES == 2 * 258 * 4 + 2 * 8
    assert metrics.NOREF_COLUMNS == ref.COLUMNS


def test_scratch_size_is_one_record_per_tile():
    q = cabi_ledger.library().load().cfen_noref_bytes
    from cfen_vit_dehazing_amd import ops
    tw, th, rec = ops.NOREF_TILE_W, ops.NOREF_TILE_H, ops.NOREF_RECORD_BYTES
    for B, H, W in ((1, 1, 1), (2, 3, 5), (3, 17, 67), (1, th, tw), (1, th + 1, tw), (1, th, tw + 1), (2, 97, 131), (8, 512, 512), (1, 2160, 3840),
                    (65535, 65536, 65536)):
        for r in (0, 7, 16):
            assert q(B, H, W, r) == B * -(-H // th) * -(-W // tw) * rec, (B, H, W, r)
    for B, H, W, r in ((0, 4, 4, 7), (-1, 4, 4, 7), (65536, 4, 4, 7), (1, 0, 4, 7), (1, 4, 0, 7), (1, 65537, 4, 7), (1, 4, 65537, 7), (1, 4, 4, -1),
                       (1, 4, 4, 17)):
        assert q(B, H, W, r) == 0, (B, H, W, r)


def test_argument_errors_do_not_need_a_gpu():
    lib = cabi_ledger.library().load()
    hz, out, scr, cnt, grd, d0, d1, z = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, (6 << 20) + 1, (7 << 20) + 3, 0))
    refused = functools.partial(cabi_ledger.refused, lib, "noref_u8")

    for bad in ((z, out, scr, cnt, grd), (hz, z, scr, cnt, grd), (hz, out, z, cnt, grd), (hz, out, scr, z, grd), (hz, out, scr, cnt, z)):
        refused(b"null pointer", bad[0], bad[1], 1, 4, 4, 7, bad[2], bad[3], bad[4], d0, d1, z)
    refused(b"B = 0", hz, out, 0, 4, 4, 7, scr, cnt, grd, d0, d1, z)
    refused(b"B = -3", hz, out, -3, 4, 4, 7, scr, cnt, grd, d0, d1, z)
    refused(b"B = 65536", hz, out, 65536, 4, 4, 7, scr, cnt, grd, d0, d1, z)
    refused(b"H = 0", hz, out, 1, 0, 4, 7, scr, cnt, grd, d0, d1, z)
    refused(b"W = 0", hz, out, 1, 4, 0, 7, scr, cnt, grd, d0, d1, z)
    refused(b"H = 65537", hz, out, 1, 65537, 4, 7, scr, cnt, grd, d0, d1, z)
    refused(b"W = 65537", hz, out, 1, 4, 65537, 7, scr, cnt, grd, d0, d1, z)
    refused(b"radius = -1", hz, out, 1, 4, 4, -1, scr, cnt, grd, d0, d1, z)
    refused(b"radius = 17", hz, out, 1, 4, 4, 17, scr, cnt, grd, d0, d1, z)
    for k in range(3):
        args = [scr, cnt, grd]
        args[k] = ctypes.c_void_p(args[k].value + 4)
        refused(b"8-byte aligned", hz, out, 1, 4, 4, 7, args[0], args[1], args[2], z, z, z)


# ---- options -----------------------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ckpt"), "--gpu_ids", "-1"] + extra)


def test_eval_noref_options(tmp_path, capsys):
    with pytest.raises(ValueError, match="--eval_noref needs --sb"):
        _parse(tmp_path, ["--eval_noref"])
    with pytest.raises(ValueError, match="--eval_noref.*needs --in_flight 1"):
        _parse(tmp_path, ["--sb", "--eval_noref", "--in_flight", "2"])
    with pytest.raises(ValueError, match="--noref_radius.*needs --eval_noref"):
        _parse(tmp_path, ["--sb", "--noref_radius", "3"])
    for bad in ("-1", "17"):
        with pytest.raises(ValueError, match=r"--noref_radius must be in 0 \.\. 16"):
            _parse(tmp_path, ["--sb", "--eval_noref", "--noref_radius", bad])
    capsys.readouterr()
    opt = _parse(tmp_path, ["--sb", "--eval_noref"])                      # no --eval, no clear/, no --gt_dir
    assert opt.eval_noref is True and opt.noref_radius == 7 and opt.eval is False
    keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
    assert "eval_noref" in keys and "noref_radius" in keys and "eval" not in keys
    for r in (0, 16):
        assert _parse(tmp_path, ["--sb", "--eval_noref", "--noref_radius", str(r)]).noref_radius == r
    opt = _parse(tmp_path, ["--sb", "--eval_noref", "--eval", "--eval_ciede2000", "--tile", "--self_ensemble", "--gpu_png", "--precision", "half"])
    assert opt.eval_noref and opt.eval and opt.eval_metrics == "psnr,ssim"
    opt = _parse(tmp_path, ["--sb", "--eval_noref", "--fit", "--fit_refine", "guided", "--u8_input", "--batchSize", "2"])
    assert opt.eval_noref and opt.fit
    capsys.readouterr()
    for extra in (["--sb", "--eval"], ["--sb"]):
        opt = _parse(tmp_path, extra)
        assert opt.eval_noref is False
        keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
        assert "eval_noref" not in keys and "noref_radius" not in keys and "tile" in keys      # a run without the flag prints the options it always printed
        saved = [line.split(":")[0] for line in open(tmp_path / "ckpt" / opt.name / "opt.txt").read().splitlines()]
        assert "eval_noref" not in saved and "noref_radius" not in saved
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    o = TestOptions()
    o.initialize()
    for flag in ("--eval_noref", "--noref_radius"):
        action = next(a for a in o.parser._actions if flag in a.option_strings)
        assert action.help.startswith("(extension)")


# ---- csv -----------------------------------------------------------------------------------------------------------------------------------------------
def test_csv_text_and_summary():
    from cfen_vit_dehazing_amd import metrics
    assert metrics.NOREF_CSV_HEADER == ("image,dark_in,dark_out,entropy_in,entropy_out,avg_gradient_in,avg_gradient_out,contrast_in,contrast_out,"
                                        "saturated")
    rows = [("a.png", 0.5, 0.25, 7.1234567, 7.5, 3.0, 5.0, 0.2, 0.3, 0.01),
            ("b.png", 0.7, 0.35, 6.0, 6.5, float("nan"), float("nan"), 0.1, 0.2, 0.0)]
    assert metrics.format_noref_csv(rows) == (metrics.NOREF_CSV_HEADER + "\n"
                                              "a.png,0.500000,0.250000,7.123457,7.500000,3.000000,5.000000,0.200000,0.300000,0.010000\n"
                                              "b.png,0.700000,0.350000,6.000000,6.500000,nan,nan,0.100000,0.200000,0.000000\n")
    assert metrics.format_noref_csv([]) == metrics.NOREF_CSV_HEADER + "\n"
    assert metrics.noref_summary_line(rows) == ("noref: 2 images, mean dark channel 0.600000 -> 0.300000, mean entropy 6.5617 -> 7.0000, "
                                                "mean avg gradient 3.0000 -> 5.0000, mean saturated 0.005000")
    s = metrics.summarize_noref(rows)
    assert s["images"] == 2 and abs(s["contrast_out_mean"] - 0.25) < 1e-15 and s["avg_gradient_in_mean"] == 3.0
    assert math.isnan(metrics.summarize_noref([])["dark_in_mean"]) and metrics.noref_summary_line([]).startswith("noref: 0 images, mean dark channel nan")
    with pytest.raises(ValueError):
        metrics.format_noref_csv([("a.png", 1.0, 2.0)])


def test_noref_from_stats_refuses_a_histogram_of_another_size():
    from cfen_vit_dehazing_amd import metrics
    img = np.zeros((1, 4, 5, 3), np.uint8)
    counts, grad, _ = ref.stats(img, img, 1)
    with pytest.raises(ValueError, match="histogram"):
        metrics.noref_from_stats(counts, grad, 4, 6)
    import torch
    rows = metrics.noref_from_stats(torch.from_numpy(counts.copy()), torch.from_numpy(grad.copy()), 4, 5)      # tensors as well as arrays
    assert rows == metrics.noref_from_stats(counts.tolist(), grad.tolist(), 4, 5)


def test_noref_needs_cuda_tensors():
    import torch
    from cfen_vit_dehazing_amd import metrics
    z = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="noref needs CUDA tensors; there is no CPU fallback"):
        metrics.noref(z, z)
    with pytest.raises(ValueError, match="noref needs CUDA tensors"):
        metrics.noref(z.numpy(), z.numpy())


# ---- the hazy bytes from the loader's floats -------------------------------------------------------------------------------------------------------
def test_every_byte_comes_back_from_the_normalised_floats():
    import torch
    from PIL import Image
    from cfen_vit_dehazing_amd import metrics
    from cfen_vit_dehazing_amd.data import to_normalized_tensor
    from cfen_vit_dehazing_amd.util import util
    v = np.arange(256, dtype=np.uint8)
    img = np.stack([v.reshape(16, 16), v[::-1].reshape(16, 16), np.roll(v, 77).reshape(16, 16)], -1)
    x = to_normalized_tensor(Image.fromarray(img))[None]                    # what the loader hands over without --u8_input
    back = metrics.bytes_from_normalized(x)
    assert back.dtype == torch.uint8 and tuple(back.shape) == (1, 16, 16, 3) and back.is_contiguous()
    assert np.array_equal(back[0].numpy(), img)                             # all 256 values, in every channel
    truncated = util.tensor2im(x[0])                                          # the reference's way back truncates: some values come back one level low
    assert truncated.shape == img.shape and (truncated.astype(int) - img).min() == -1 and (truncated != img).any()
