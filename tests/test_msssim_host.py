"""MS-SSIM scoring (cfen_image_msssim, metrics.py, test.py --eval --eval_metrics psnr,ssim,msssim): everything that can be checked without a GPU --
the fixture tests/golden/msssim_pairs.npz against its float64 restatement (tests/msssim_ref.py), the host-side combination and its NaN rule, csv
and summary text for three and four columns, option refusals, the size check of the dataset and the C ABI's argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest

import metrics_images as mi
import msssim_ref as mr


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "msssim_pairs.npz"))


def test_fixture_covers_the_cases_and_the_images_regenerate_bit_identically(fixture):
    assert [str(n) for n in fixture["names"]] == list(mr.CASES)
    for k, name in enumerate(mr.CASES):
        a, b = mr.pair(name)
        assert a.dtype == np.uint8 and a.shape == (mr.CASES[name][0],) + mr.CASES[name][1:3] + (3,)
        assert mi.crc(a) == int(fixture["crc_a"][k]) and mi.crc(b) == int(fixture["crc_b"][k]), name
        assert int(fixture["offsets"][k + 1] - fixture["offsets"][k]) == a.shape[0]
    n = int(fixture["offsets"][-1])
    assert fixture["ref32_levels"].shape == fixture["f64_levels"].shape == (n, 5, 2) and fixture["ref32_ms"].shape == fixture["f64_ms"].shape == (n,)


def test_float64_restatement_agrees_with_the_reference_values(fixture):
    """the reference runs in fp32: its level values and its MS-SSIM sit within the stored distances of the float64 restatement recomputed here"""
    d_level, d_nan, d_ms = float(fixture["D_level"]), float(fixture["D_level_nan"]), float(fixture["D_ms"])
    assert 0 < d_level < 1e-4 and 0 < d_nan < 1e-3 and 0 < d_ms < 1e-5
    for k, name in enumerate(mr.CASES):
        if name == "512x512_batch8":
            continue                      # (recomputed by the GPU test; the stored values are checked below all the same)
        a, b = mr.pair(name)
        for i in range(a.shape[0]):
            j = int(fixture["offsets"][k]) + i
            got = mr.levels_f64_u8(a[i], b[i])
            assert np.abs(got - fixture["f64_levels"][j]).max() <= 1e-12, name
            assert np.abs(got - fixture["ref32_levels"][j]).max() <= (d_nan if name == "anticorrelated_176" else d_level), name
            ms = mr.combine(got)
            if name == "anticorrelated_176":
                assert math.isnan(ms) and math.isnan(fixture["f64_ms"][j]) and math.isnan(fixture["ref32_ms"][j])
            else:
                assert abs(ms - fixture["f64_ms"][j]) <= 1e-12 and abs(ms - fixture["ref32_ms"][j]) <= d_ms, name
            assert mi.sse_int(a[i], b[i]) == int(fixture["sse"][j])
    finite = np.isfinite(fixture["f64_ms"])
    assert np.abs(fixture["ref32_levels"] - fixture["f64_levels"]).reshape(len(finite), -1).max(axis=1).tolist() == fixture["D_level_pair"].tolist()
    assert fixture["D_level_pair"][finite].max() == d_level and fixture["D_level_pair"][~finite].max() == d_nan
    assert np.abs(fixture["ref32_ms"] - fixture["f64_ms"])[finite].max() == d_ms


def test_the_special_pairs_are_what_their_names_say(fixture):
    names = list(mr.CASES)
    j = int(fixture["offsets"][names.index("identical_176")])
    assert (fixture["f64_levels"][j] == 1.0).all() and (fixture["ref32_levels"][j] == 1.0).all() and fixture["f64_ms"][j] == 1.0 and fixture["sse"][j] == 0
    j = int(fixture["offsets"][names.index("black_white_176")])
    assert np.abs(fixture["f64_levels"][j, :, 1] - 1.0).max() <= 1e-12 and 0 < fixture["f64_ms"][j] < 1           # cs = C2 / C2, ssim = C1 / (1 + C1)
    assert fixture["sse"][j] == 255 ** 2 * 176 * 176 * 3
    j = int(fixture["offsets"][names.index("anticorrelated_176")])
    lv = fixture["f64_levels"][j]
    assert np.isfinite(lv).all() and lv[:4, 1].min() < 0 and math.isnan(fixture["f64_ms"][j])
    finite = np.isfinite(fixture["f64_ms"])
    assert finite.sum() == len(finite) - 1 and fixture["f64_levels"][finite][:, :, 1].min() > 0.8


def test_pooling_floors_odd_sizes():
    x = np.arange(5 * 7, dtype=np.float64).reshape(1, 5, 7)
    p = mr.pool2(x)
    assert p.shape == (1, 2, 3) and p[0, 0, 0] == (0 + 1 + 7 + 8) / 4 and p[0, 1, 2] == (18 + 19 + 25 + 26) / 4
    sizes = [(177, 203)]
    for _ in range(4):
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    assert sizes == [(177, 203), (88, 101), (44, 50), (22, 25), (11, 12)]
    with pytest.raises(ValueError, match="176"):
        mr.levels_f64(np.zeros((3, 175, 300)), np.zeros((3, 175, 300)))


# ---- host combination ------------------------------------------------------------------------------------------------------------------------
def test_msssim_from_levels_on_the_fixture(fixture):
    from cfen_vit_dehazing_amd import metrics
    assert metrics.MSSSIM_WEIGHTS == mr.WEIGHTS and metrics.MSSSIM_MIN_EDGE == mr.MIN_EDGE
    got = metrics.msssim_from_levels(fixture["f64_levels"])
    assert isinstance(got, list) and len(got) == len(fixture["f64_ms"])
    for g, want in zip(got, fixture["f64_ms"]):
        assert (math.isnan(g) and math.isnan(want)) or abs(g - want) <= 1e-15
    # from the reference's own fp32 level values: its combined value, up to its five fp32 powers (weights rounded to fp32 too) and five products --
    # some fifteen roundings of 2^-24 relative on a value under 1: 1e-6
    got = metrics.msssim_from_levels(fixture["ref32_levels"].tolist())
    for g, want in zip(got, fixture["ref32_ms"]):
        assert (math.isnan(g) and math.isnan(want)) or abs(g - want) <= 1e-6
    one = metrics.msssim_from_levels(fixture["f64_levels"][0])
    assert isinstance(one, float) and one == metrics.msssim_from_levels(fixture["f64_levels"][:1])[0]
    import torch
    assert metrics.msssim_from_levels(torch.from_numpy(fixture["f64_levels"][:3])) == metrics.msssim_from_levels(fixture["f64_levels"][:3])


def test_msssim_from_levels_nan_rule():
    from cfen_vit_dehazing_amd import metrics
    ones = [[1.0, 1.0]] * 5
    assert metrics.msssim_from_levels(ones) == 1.0 and metrics.msssim_from_levels([ones, ones]) == [1.0, 1.0]
    for l in range(4):                                  # a negative cs_l at a used level
        lv = [list(p) for p in ones]
        lv[l][1] = -0.25
        assert math.isnan(metrics.msssim_from_levels(lv))
        lv[l][1] = 0.0
        assert metrics.msssim_from_levels(lv) == 0.0
    lv = [list(p) for p in ones]
    lv[4][1] = -0.5                                     # cs_4 and ssim_0 .. ssim_3 are not used
    for l in range(4):
        lv[l][0] = -0.5
    assert metrics.msssim_from_levels(lv) == 1.0
    lv[4][0] = -1e-9
    assert math.isnan(metrics.msssim_from_levels(lv))
    lv[4][0] = float("nan")
    assert math.isnan(metrics.msssim_from_levels(lv))
    half = [[0.5, 0.5]] * 5
    assert abs(metrics.msssim_from_levels(half) - 0.5 ** sum(mr.WEIGHTS)) <= 1e-15
    with pytest.raises(ValueError):
        metrics.msssim_from_levels([[[1.0, 1.0]] * 4])
    with pytest.raises(ValueError, match="CUDA"):
        import torch
        metrics.psnr_ssim_msssim(torch.zeros(176, 176, 3, dtype=torch.uint8), torch.zeros(176, 176, 3, dtype=torch.uint8))


# ---- csv ---------------------------------------------------------------------------------------------------------------------------------
def test_csv_text_and_summary_for_three_and_four_columns():
    from cfen_vit_dehazing_amd import metrics
    rows3 = [("1400_1.png", 23.4567891, 0.9123456789), ("same.png", float("inf"), 1.0), ("b.png", 10.0, 0.5)]
    two = ("psnr", "ssim")
    assert metrics.CSV_HEADER == "image,psnr,ssim" == metrics.csv_header(two)
    assert metrics.format_csv_columns(rows3, two) == metrics.format_csv(rows3) == \
        "image,psnr,ssim\n1400_1.png,23.456789,0.912346\nsame.png,inf,1.000000\nb.png,10.000000,0.500000\n"
    assert metrics.summary_line_columns(rows3, two) == metrics.summary_line(rows3) and "MS-SSIM" not in metrics.summary_line(rows3)
    assert metrics.summarize_columns(rows3, two) == metrics.summarize(rows3)
    three = ("psnr", "ssim", "msssim")
    rows4 = [("1400_1.png", 23.4567891, 0.9123456789, 0.95), ("same.png", float("inf"), 1.0, 1.0), ("b.png", 10.0, 0.5, float("nan"))]
    assert metrics.format_csv_columns(rows4, three) == \
        "image,psnr,ssim,msssim\n1400_1.png,23.456789,0.912346,0.950000\nsame.png,inf,1.000000,1.000000\nb.png,10.000000,0.500000,nan\n"
    assert metrics.format_csv_columns([], three) == "image,psnr,ssim,msssim\n"
    s = metrics.summarize_columns(rows4, three)
    assert s["images"] == 3 and s["psnr_infinite"] == 1 and s["msssim_nan"] == 1 and abs(s["msssim_mean"] - 0.975) < 1e-12
    assert abs(s["ssim_mean"] - (0.9123456789 + 1.0 + 0.5) / 3) < 1e-12
    line = metrics.summary_line_columns(rows4, three)
    assert line.startswith(metrics.summary_line(rows3)) and line.endswith(", mean MS-SSIM 0.975000 over 2 (1 nan)")
    assert math.isnan(metrics.summarize_columns([("x", 1.0, 1.0, float("nan"))], three)["msssim_mean"])
    with pytest.raises(ValueError):
        metrics.format_csv_columns(rows3, three)


# ---- options -----------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ckpt"), "--gpu_ids", "-1"] + extra)


def test_eval_metrics_needs_eval_and_known_names(tmp_path, capsys):
    with pytest.raises(ValueError, match="needs --eval"):
        _parse(tmp_path, ["--sb", "--eval_metrics", "psnr,ssim,msssim"])
    with pytest.raises(ValueError, match="needs --eval"):
        _parse(tmp_path, ["--sb", "--eval_metrics", "psnr,ssim"])
    with pytest.raises(ValueError, match="ciede2000"):
        _parse(tmp_path, ["--sb", "--eval", "--eval_metrics", "psnr,ssim,ciede2000"])
    with pytest.raises(ValueError, match="psnr and ssim"):
        _parse(tmp_path, ["--sb", "--eval", "--eval_metrics", "msssim"])
    capsys.readouterr()
    opt = _parse(tmp_path, ["--sb", "--eval", "--eval_metrics", "msssim,psnr,ssim"])
    assert opt.eval_metrics == "psnr,ssim,msssim"                       # the csv's order, whatever the flag's
    assert "eval_metrics: psnr,ssim,msssim" in capsys.readouterr().out
    opt = _parse(tmp_path, ["--sb", "--eval"])
    assert opt.eval_metrics == "psnr,ssim"
    keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
    assert "eval" in keys and "eval_metrics" not in keys                # a run without the flag prints the options it always printed
    opt = _parse(tmp_path, ["--sb"])
    keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
    assert "tile" in keys and "eval_metrics" not in keys and "eval" not in keys
    assert "eval_metrics" not in [line.split(":")[0] for line in open(tmp_path / "ckpt" / opt.name / "opt.txt").read().splitlines()]


def _touch_png(path, size):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros((size[1], size[0], 3), dtype=np.uint8)).save(path)


def test_an_image_under_176_is_named_when_the_dataset_is_built(tmp_path):
    from types import SimpleNamespace
    from cfen_vit_dehazing_amd.data import DECVITDATA
    for n, size in (("big_1.png", (240, 180)), ("small_1.png", (300, 175))):         # (width, height)
        _touch_png(str(tmp_path / "hazy" / n), size)
        _touch_png(str(tmp_path / "clear" / n.replace("_1", "")), size)
    opt = SimpleNamespace(dataroot=str(tmp_path), sb=True, resize_or_crop="resize", u8_input=False, eval=True, gt_dir=None, output_nc=3, input_nc=3,
                          which_direction="AtoB", eval_metrics="psnr,ssim,msssim")
    with pytest.raises(ValueError) as e:
        DECVITDATA().initialize(opt)
    assert "small_1.png" in str(e.value) and "176" in str(e.value) and "175 x 300" in str(e.value) and "big_1.png" not in str(e.value)
    opt.eval_metrics = "psnr,ssim"
    DECVITDATA().initialize(opt)                     # PSNR / SSIM alone take any image from 11 x 11 up
    os.remove(tmp_path / "hazy" / "small_1.png")
    opt.eval_metrics = "psnr,ssim,msssim"
    ds = DECVITDATA()
    ds.initialize(opt)
    assert len(ds) == 1 and tuple(ds[0]["A"].shape) == (180, 240, 3)


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_declared_exported_and_bound():
    from cfen_vit_dehazing_amd import _lib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cfen_hip.h")).read()
    lib = _lib.load()
    for sym in ("cfen_image_msssim_bytes", "cfen_image_msssim"):
        assert sym + "(" in text and sym in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert _lib.SIGNATURES["cfen_image_msssim"] == _lib.SIGNATURES["cfen_image_metrics"]
    assert lib.cfen_abi_version() == 1


def test_argument_errors_are_caught_on_the_host():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    P, S = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    call = lambda u8, a, b, B, C, H, W, lo, hi, scratch, out: lib.cfen_image_msssim(u8, a, b, B, C, H, W, lo, hi, scratch, out, S)
    assert call(1, P, P, 1, 3, 175, 300, 0.0, 1.0, P, P) == -1 and b"176" in lib.cfen_last_error()
    assert call(1, P, P, 1, 3, 300, 175, 0.0, 1.0, P, P) == -1 and b"176" in lib.cfen_last_error()
    assert call(0, P, P, 1, 2, 256, 256, 0.0, 1.0, P, P) == -1 and b"C = 2" in lib.cfen_last_error()
    assert call(1, P, P, 1, 1, 256, 256, 0.0, 1.0, P, P) == -1                                               # uint8 images are RGB
    assert call(1, P, P, 1, 3, 256, 256, 0.0, 1.0, P, ctypes.c_void_p(0)) == -1 and b"null" in lib.cfen_last_error()
    assert call(1, ctypes.c_void_p(0), P, 1, 3, 256, 256, 0.0, 1.0, P, P) == -1
    assert call(1, P, P, 1, 3, 256, 256, 0.0, 1.0, ctypes.c_void_p(0), P) == -1
    assert call(1, P, P, 1, 3, 256, 256, 0.0, 1.0, P, ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.cfen_last_error()
    assert call(0, P, P, 1, 3, 256, 256, 1.0, 1.0, P, P) == -1 and b"range" in lib.cfen_last_error()
    assert call(2, P, P, 1, 3, 256, 256, 0.0, 1.0, P, P) == -1
    assert call(1, P, P, 0, 3, 256, 256, 0.0, 1.0, P, P) == -1


def _want_bytes(B, C, H, W):
    """every level's (sse, ssim sum, cs sum) per 24 x 64 tile in doubles, then levels 1 .. 4 of both images in fp32, rounded up to 16"""
    doubles = floats = 0
    for l in range(5):
        doubles += B * -(-(H - 10) // 24) * -(-(W - 10) // 64) * 3
        if l:
            floats += 2 * B * C * H * W
        H, W = H // 2, W // 2
    return -(-(doubles * 8 + floats * 4) // 16) * 16


def test_scratch_size_is_the_pyramid_plus_the_partials():
    from cfen_vit_dehazing_amd import _lib
    q = _lib.load().cfen_image_msssim_bytes
    for B, C, H, W in ((1, 3, 176, 176), (2, 3, 177, 203), (1, 3, 200, 330), (8, 3, 512, 512), (1, 1, 512, 512), (1, 3, 2160, 3840), (3, 3, 65536, 65536)):
        assert q(B, C, H, W) == _want_bytes(B, C, H, W), (B, C, H, W)
    assert q(1, 3, 175, 300) == 0 and q(1, 3, 300, 175) == 0 and q(1, 2, 256, 256) == 0 and q(0, 3, 256, 256) == 0 and q(1, 3, 176, 65537) == 0
