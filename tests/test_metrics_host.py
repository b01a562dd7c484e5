"""PSNR / SSIM scoring (csrc/k_metrics.hip, metrics.py, test.py --eval): everything that can be checked without a GPU -- the fixture
tests/golden/metrics_pairs.npz against its float64 restatement, the regenerated images, ground-truth pairing, option refusals, csv text and the
C ABI's argument checks."""
import ctypes
import math
import os

import numpy as np
import pytest

import metrics_images as mi


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_pairs.npz"))


def test_fixture_covers_the_cases_and_the_images_regenerate_bit_identically(fixture):
    assert [str(n) for n in fixture["names"]] == list(mi.CASES)
    for k, name in enumerate(mi.CASES):
        a, b = mi.pair(name)
        assert a.dtype == np.uint8 and a.shape == (mi.CASES[name][0],) + mi.CASES[name][1:3] + (3,)
        assert mi.crc(a) == int(fixture["crc_a"][k]) and mi.crc(b) == int(fixture["crc_b"][k]), name
        assert int(fixture["offsets"][k + 1] - fixture["offsets"][k]) == a.shape[0]


def test_float64_restatement_agrees_with_the_reference_values(fixture):
    """the reference runs in fp32: its values sit within the stored distance max |ref32 - f64| of the float64 restatement recomputed here"""
    dist = float(fixture["max_ref32_f64"])
    assert 0 < dist < 1e-4
    for k, name in enumerate(mi.CASES):
        if mi.CASES[name][1] > 600:
            continue                      # (the 1080p pair is recomputed by the GPU test; the stored f64 value is checked below all the same)
        a, b = mi.pair(name)
        for i in range(a.shape[0]):
            j = int(fixture["offsets"][k]) + i
            got = mi.ssim_f64_u8(a[i], b[i])
            assert abs(got - float(fixture["f64"][j])) <= 1e-12, name
            assert abs(got - float(fixture["ref32"][j])) <= dist, name
            assert mi.sse_int(a[i], b[i]) == int(fixture["sse"][j])
    assert np.abs(fixture["ref32"] - fixture["f64"]).max() == dist
    j = int(fixture["offsets"][list(mi.CASES).index("identical_64x64")])
    assert fixture["f64"][j] == 1.0 and fixture["sse"][j] == 0
    assert mi.psnr_from_sse(0, 10) == float("inf")


# ---- pairing -----------------------------------------------------------------------------------------------------------------------------
def _touch_png(path, size=(16, 12)):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros((size[1], size[0], 3), dtype=np.uint8)).save(path)


def test_ground_truth_pairing_same_stem_then_reside_prefix(tmp_path):
    from cfen_vit_dehazing_amd.data import pair_ground_truth
    hazy = [str(tmp_path / "hazy" / n) for n in ("scene.png", "1400_1.png", "1400_2_0.16.png", "a_b.jpg")]
    for n in ("scene.jpg", "1400.png", "a_b.png", "a.png"):
        _touch_png(str(tmp_path / "clear" / n))
    got = pair_ground_truth(hazy, str(tmp_path / "clear"))
    assert [os.path.basename(got[h]) for h in hazy] == ["scene.jpg", "1400.png", "1400.png", "a_b.png"]      # the full stem wins over the prefix


def test_a_hazy_image_without_a_partner_is_named_when_the_dataset_is_built(tmp_path):
    from types import SimpleNamespace
    from cfen_vit_dehazing_amd.data import DECVITDATA
    for n in ("1400_1.png", "orphan_7.png"):
        _touch_png(str(tmp_path / "hazy" / n))
    _touch_png(str(tmp_path / "clear" / "1400.png"))
    opt = SimpleNamespace(dataroot=str(tmp_path), sb=True, resize_or_crop="resize", u8_input=False, eval=True, gt_dir=None, output_nc=3, input_nc=3,
                          which_direction="AtoB")
    with pytest.raises(ValueError, match="orphan_7.png"):
        DECVITDATA().initialize(opt)
    opt.eval = False
    ds = DECVITDATA()
    ds.initialize(opt)                       # without --eval nobody looks for ground truth
    assert sorted(ds[0]) == ["B", "B_paths"]
    with pytest.raises(ValueError, match="does not exist"):
        DECVITDATA().initialize(SimpleNamespace(**dict(vars(opt), eval=True, gt_dir=str(tmp_path / "nowhere"))))


def test_a_ground_truth_of_another_size_names_both_files(tmp_path):
    from types import SimpleNamespace
    from cfen_vit_dehazing_amd.data import DECVITDATA
    _touch_png(str(tmp_path / "hazy" / "5_1.png"), size=(16, 12))
    _touch_png(str(tmp_path / "hazy" / "6_1.png"), size=(16, 12))
    _touch_png(str(tmp_path / "gt" / "5.png"), size=(16, 12))
    _touch_png(str(tmp_path / "gt" / "6.png"), size=(12, 16))
    for u8 in (False, True):
        opt = SimpleNamespace(dataroot=str(tmp_path), sb=True, resize_or_crop="resize", u8_input=u8, eval=True, gt_dir=str(tmp_path / "gt"), output_nc=3,
                              input_nc=3, which_direction="AtoB")
        ds = DECVITDATA()
        ds.initialize(opt)
        item = ds[0]
        assert item["A"].dtype.is_floating_point is False and tuple(item["A"].shape) == (12, 16, 3) and item["A_paths"].endswith("5.png")
        with pytest.raises(ValueError) as e:
            ds[1]
        assert "6.png" in str(e.value) and "6_1.png" in str(e.value) and "16 x 12" in str(e.value) and "12 x 16" in str(e.value)


# ---- options -----------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ckpt"), "--gpu_ids", "-1"] + extra)


def test_eval_is_refused_with_the_pipelined_driver_and_without_sb(tmp_path, capsys):
    with pytest.raises(ValueError, match="--in_flight 1"):
        _parse(tmp_path, ["--eval", "--sb", "--in_flight", "2"])
    with pytest.raises(ValueError, match="--sb"):
        _parse(tmp_path, ["--eval"])
    opt = _parse(tmp_path, ["--eval", "--sb"])
    assert opt.eval and opt.gt_dir is None
    assert "eval: True" in capsys.readouterr().out
    opt = _parse(tmp_path, ["--sb"])
    assert not opt.eval
    out = capsys.readouterr().out
    keys = [line.split(":")[0] for line in out.splitlines()]
    assert "tile" in keys and "eval" not in keys and "gt_dir" not in keys       # a run without --eval prints the options it always printed


# ---- csv ---------------------------------------------------------------------------------------------------------------------------------
def test_csv_text_and_summary():
    from cfen_vit_dehazing_amd import metrics
    rows = [("1400_1.png", 23.4567891, 0.9123456789), ("same.png", float("inf"), 1.0), ("b.png", 10.0, 0.5)]
    assert metrics.format_csv(rows) == "image,psnr,ssim\n1400_1.png,23.456789,0.912346\nsame.png,inf,1.000000\nb.png,10.000000,0.500000\n"
    assert metrics.format_csv([]) == "image,psnr,ssim\n"
    s = metrics.summarize(rows)
    assert s["images"] == 3 and s["psnr_infinite"] == 1 and abs(s["psnr_mean"] - (23.4567891 + 10.0) / 2) < 1e-12
    assert abs(s["ssim_mean"] - (0.9123456789 + 1.0 + 0.5) / 3) < 1e-12
    assert "1 infinite" in metrics.summary_line(rows)
    assert math.isnan(metrics.summarize([("x", float("inf"), 1.0)])["psnr_mean"])
    assert metrics.psnr_from_sse(0, 100) == float("inf")
    assert abs(metrics.psnr_from_sse(255 ** 2 * 100, 100)) < 1e-12           # MSE 1 on the [0,1] scale: 0 dB
    assert abs(metrics.psnr_from_sse(650.25, 1000) - 50.0) < 1e-9             # 255^2 * 1000 / 650.25 = 1e5
    with pytest.raises(ValueError, match="CUDA"):
        import torch
        metrics.psnr_ssim(torch.zeros(11, 11, 3, dtype=torch.uint8), torch.zeros(11, 11, 3, dtype=torch.uint8))


# ---- C ABI -------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_caught_on_the_host():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    P, S = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    call = lambda u8, a, b, B, C, H, W, lo, hi, scratch, out: lib.cfen_image_metrics(u8, a, b, B, C, H, W, lo, hi, scratch, out, S)
    assert call(1, P, P, 1, 3, 10, 64, 0.0, 1.0, P, P) == -1 and b"11 x 11" in lib.cfen_last_error()      # H = 10
    assert call(1, P, P, 1, 3, 64, 10, 0.0, 1.0, P, P) == -1
    assert call(0, P, P, 1, 2, 64, 64, 0.0, 1.0, P, P) == -1 and b"C = 2" in lib.cfen_last_error()
    assert call(1, P, P, 1, 1, 64, 64, 0.0, 1.0, P, P) == -1                                                # uint8 images are RGB
    assert call(1, P, P, 1, 3, 64, 64, 0.0, 1.0, P, ctypes.c_void_p(0)) == -1 and b"null" in lib.cfen_last_error()
    assert call(1, ctypes.c_void_p(0), P, 1, 3, 64, 64, 0.0, 1.0, P, P) == -1
    assert call(1, P, P, 1, 3, 64, 64, 0.0, 1.0, ctypes.c_void_p(0), P) == -1
    assert call(1, P, P, 1, 3, 64, 64, 0.0, 1.0, P, ctypes.c_void_p(4100)) == -1 and b"aligned" in lib.cfen_last_error()
    assert call(0, P, P, 1, 3, 64, 64, 1.0, 1.0, P, P) == -1 and b"range" in lib.cfen_last_error()
    assert call(0, P, P, 1, 3, 64, 64, 0.0, float("nan"), P, P) == -1
    assert call(2, P, P, 1, 3, 64, 64, 0.0, 1.0, P, P) == -1
    assert call(1, P, P, 0, 3, 64, 64, 0.0, 1.0, P, P) == -1
    assert lib.cfen_abi_version() == 1


def test_scratch_size_is_positive_and_monotone():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    q = lib.cfen_image_metrics_bytes
    assert q(1, 3, 11, 11) > 0 and q(1, 3, 11, 11) % 16 == 0
    edges = [11, 12, 34, 35, 37, 53, 64, 74, 75, 480, 512, 640, 1080, 1920, 2160, 3840]
    for fixed in (11, 512, 3840):                                 # never smaller for a larger image, in either dimension
        for vals in ([q(1, 3, e, fixed) for e in edges], [q(1, 3, fixed, e) for e in edges]):
            assert all(v > 0 for v in vals) and vals == sorted(vals)
    assert [q(b, 3, 64, 64) for b in (1, 2, 3, 8)] == sorted(q(b, 3, 64, 64) for b in (1, 2, 3, 8))
    assert q(8, 3, 512, 512) == 8 * q(1, 3, 512, 512)
    assert q(1, 1, 512, 512) == q(1, 3, 512, 512)            # one partial pair per tile, whatever the channel count
    assert q(1, 3, 10, 64) == 0 and q(1, 2, 64, 64) == 0 and q(0, 3, 64, 64) == 0     # what the launch refuses needs no scratch
