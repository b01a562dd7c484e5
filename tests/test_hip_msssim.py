"""MS-SSIM on the device (cfen_image_msssim, ops.image_msssim, metrics.psnr_ssim_msssim, test.py --eval --eval_metrics psnr,ssim,msssim) against
the reference's pytorch_msssim values and their float64 restatement (tests/golden/msssim_pairs.npz, tests/msssim_ref.py).

Bars, by the rule of test_hip_metrics.py.  The reference itself runs in fp32; the fixture stores its own distance from float64: D_level = max
|ref32 - f64| over the ten level values of every pair with a finite MS-SSIM, D_ms the same for the combined value.  The kernel also works in fp32
with another summation order, so every level value must be within 2 D_level of float64 and 3 D_level of the reference, the combined value within
2 D_ms and 3 D_ms.  The anticorrelated pair (cs_l near -1 over small denominators, MS-SSIM NaN) is where the reference's own rounding is ten times
larger; it is held to its own distance D_level_nan and does not loosen the bar of the others.  Identical images must give exactly 1.0 at every
level.  The squared error of uint8 input is exact.  The worst measured differences go to profiles/msssim_parity.json (CFEN_WRITE_PARITY=1)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import metrics, ops
from cfen_vit_dehazing_amd._lib import CfenError
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import metrics_images as mi
import msssim_ref as mr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}
_PAIRS = {}


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "msssim_pairs.npz"))


def _pair(name):
    """the regenerated images of a case on the host and on the device, made once"""
    if name not in _PAIRS:
        a, b = mr.pair(name)
        _PAIRS[name] = (a, b, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    return _PAIRS[name]


def _floats(name):
    """v / 255 in fp32, divided on the host (IEEE division, what the kernel does to bytes), as (B,3,H,W) device tensors"""
    a, b = _pair(name)[:2]
    return tuple(torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)).to(DEV) for x in (a, b))


def _record(fixture, mode, name, d64, d32, m64, m32):
    w = _WORST.setdefault(mode, {"level_worst_abs_diff_from_f64": 0.0, "level_worst_abs_diff_from_ref32": 0.0, "level_worst_case": None,
                                 "msssim_worst_abs_diff_from_f64": 0.0, "msssim_worst_abs_diff_from_ref32": 0.0,
                                 "anticorrelated_level_worst_abs_diff_from_f64": 0.0, "anticorrelated_level_worst_abs_diff_from_ref32": 0.0})
    if name == "anticorrelated_176":
        w["anticorrelated_level_worst_abs_diff_from_f64"] = max(w["anticorrelated_level_worst_abs_diff_from_f64"], d64)
        w["anticorrelated_level_worst_abs_diff_from_ref32"] = max(w["anticorrelated_level_worst_abs_diff_from_ref32"], d32)
    else:
        if d64 >= w["level_worst_abs_diff_from_f64"]:
            w["level_worst_abs_diff_from_f64"], w["level_worst_case"] = d64, name
        w["level_worst_abs_diff_from_ref32"] = max(w["level_worst_abs_diff_from_ref32"], d32)
        w["msssim_worst_abs_diff_from_f64"] = max(w["msssim_worst_abs_diff_from_f64"], m64)
        w["msssim_worst_abs_diff_from_ref32"] = max(w["msssim_worst_abs_diff_from_ref32"], m32)
    if os.environ.get("CFEN_WRITE_PARITY") == "1":
        with open(os.path.join(ROOT, "profiles", "msssim_parity.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reference_fp32_distance_D_level": float(fixture["D_level"]),
                       "reference_fp32_distance_D_level_anticorrelated": float(fixture["D_level_nan"]), "reference_fp32_distance_D_ms": float(fixture["D_ms"]),
                       "bars": "2 D from float64, 3 D from the reference", "modes": _WORST}, f, indent=1, sort_keys=True)
            f.write("\n")


def _check(mode, name, fixture, levels, rows=None):
    """levels: (B,5,2) device tensor; every level value and the combined value against both bars"""
    k = list(mr.CASES).index(name)
    lo, hi = int(fixture["offsets"][k]), int(fixture["offsets"][k + 1])
    nan_case = name == "anticorrelated_176"
    d_level, d_ms = float(fixture["D_level_nan" if nan_case else "D_level"]), float(fixture["D_ms"])
    lv = levels.cpu().numpy()
    assert lv.shape == (hi - lo, 5, 2) and lv.dtype == np.float64
    ms = metrics.msssim_from_levels(levels)
    for i in range(hi - lo):
        d64 = float(np.abs(lv[i] - fixture["f64_levels"][lo + i]).max())
        d32 = float(np.abs(lv[i] - fixture["ref32_levels"][lo + i]).max())
        m64 = m32 = 0.0
        if not nan_case:
            m64, m32 = abs(ms[i] - float(fixture["f64_ms"][lo + i])), abs(ms[i] - float(fixture["ref32_ms"][lo + i]))
        print("%s %s[%d]: msssim %.9f  |-f64| %.3e (bar %.3e)  |-ref32| %.3e (bar %.3e)   levels |-f64| %.3e (bar %.3e)  |-ref32| %.3e (bar %.3e)"
              % (mode, name, i, ms[i], m64, 2 * d_ms, m32, 3 * d_ms, d64, 2 * d_level, d32, 3 * d_level))
        _record(fixture, mode, name, d64, d32, m64, m32)
        assert np.isfinite(lv[i]).all()
        assert d64 <= 2 * d_level and d32 <= 3 * d_level, (mode, name, i)
        if nan_case:
            assert math.isnan(ms[i]) and lv[i, :4, 1].min() < 0
        else:
            assert m64 <= 2 * d_ms and m32 <= 3 * d_ms, (mode, name, i)
        if name == "identical_176":
            assert (lv[i] == 1.0).all() and ms[i] == 1.0
    return ms


@pytest.mark.parametrize("name", list(mr.CASES))
def test_uint8_pairs_match_the_reference_and_image_metrics_bitwise(name, fixture):
    a, b, ta, tb = _pair(name)
    sse, levels = ops.image_msssim(ta, tb)
    assert levels.shape == (a.shape[0], 5, 2) and levels.dtype == torch.float64 and levels.is_cuda and sse.shape == (a.shape[0],)
    ms = _check("uint8", name, fixture, levels)
    k = list(mr.CASES).index(name)
    want = fixture["sse"][int(fixture["offsets"][k]):int(fixture["offsets"][k + 1])]
    assert sse.cpu().tolist() == [float(w) for w in want]                                   # integer sums: exact
    m_sse, m_ssim = ops.image_metrics(ta, tb)
    assert torch.equal(sse, m_sse) and torch.equal(levels[:, 0, 0], m_ssim)                  # out[:, 0:2] is image_metrics' output, bit for bit
    rows, rows2 = metrics.psnr_ssim_msssim(ta, tb), metrics.psnr_ssim(ta, tb)
    for i, (p, s, m) in enumerate(rows):
        assert (p, s) == rows2[i]
        assert (math.isnan(m) and math.isnan(ms[i])) or m == ms[i]


@pytest.mark.parametrize("name", ["177x203_batch2", "200x330", "anticorrelated_176"])
def test_float_input_and_one_channel(name, fixture):
    a, b, ta, tb = _pair(name)
    fa, fb = _floats(name)
    u_sse, u_levels = ops.image_msssim(ta, tb)
    sse, levels = ops.image_msssim(fa, fb, value_range=(0.0, 1.0))
    assert torch.equal(levels, u_levels)                              # (v - 0) / 1 is v: the same fp32 values, the same bits at every level
    _check("float32 range (0,1)", name, fixture, levels)
    m_sse, m_ssim = ops.image_metrics(fa, fb, value_range=(0.0, 1.0))
    assert torch.equal(sse, m_sse) and torch.equal(levels[:, 0, 0], m_ssim)
    # [-1,1] data, the generator's float outputs: each value reaches the kernel within 2^-23 of v / 255 (test_hip_metrics.py); the level values move
    # by rounding only and stay inside the same bars
    na, nb = (fa - 0.5) / 0.5, (fb - 0.5) / 0.5
    sse, levels = ops.image_msssim(na, nb, value_range=(-1.0, 1.0))
    _check("float32 range (-1,1)", name, fixture, levels)
    m_sse, m_ssim = ops.image_metrics(na, nb, value_range=(-1.0, 1.0))
    assert torch.equal(sse, m_sse) and torch.equal(levels[:, 0, 0], m_ssim)
    # one channel: the means over one plane are that plane's level values
    d_level = float(fixture["D_level_nan" if name == "anticorrelated_176" else "D_level"])
    s1, l1 = ops.image_msssim(fa[:, 1:2].contiguous(), fb[:, 1:2].contiguous(), value_range=(0.0, 1.0))
    assert l1.shape == (a.shape[0], 5, 2)
    want = mr.levels_f64(fa[0, 1:2].double().cpu().numpy(), fb[0, 1:2].double().cpu().numpy())
    d = float(np.abs(l1[0].cpu().numpy() - want).max())
    print("one channel %s: levels |-f64| %.3e (bar %.3e)" % (name, d, 2 * d_level))
    assert d <= 2 * d_level


def test_batch_equals_single_calls_and_calls_repeat_bitwise():
    a, b, ta, tb = _pair("512x512_batch8")
    sse, levels = ops.image_msssim(ta, tb)
    one = [ops.image_msssim(ta[i:i + 1], tb[i:i + 1]) for i in range(8)]
    assert torch.equal(sse, torch.cat([o[0] for o in one])) and torch.equal(levels, torch.cat([o[1] for o in one]))
    again = ops.image_msssim(ta, tb)
    assert torch.equal(sse, again[0]) and torch.equal(levels, again[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.image_msssim(ta, tb)
    side.synchronize()
    assert torch.equal(sse, other[0]) and torch.equal(levels, other[1])
    _, _, oa, ob = _pair("177x203_batch2")                                 # odd extents: edge tiles at every level
    l2 = ops.image_msssim(oa, ob)[1]
    assert torch.equal(l2, torch.cat([ops.image_msssim(oa[i:i + 1], ob[i:i + 1])[1] for i in range(2)]))


@pytest.mark.parametrize("name", ["177x203_batch2", "200x330"])
def test_scratch_contents_do_not_matter(name):
    """the C ABI called directly on caller-owned scratch: filled with 0xFF bytes (NaNs as doubles and as floats) or zeroed, the same bits come out"""
    from cfen_vit_dehazing_amd import _lib
    from cfen_vit_dehazing_amd._lib import ptr, check, current_stream
    _, _, ta, tb = _pair(name)
    B, H, W, _ = ta.shape
    lib = _lib.load()
    nbytes = lib.cfen_image_msssim_bytes(B, 3, H, W)
    assert nbytes > 0 and nbytes % 16 == 0
    outs = []
    for fill in (0xFF, 0x00):
        scratch = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        out = torch.full((B, 11), float("nan"), dtype=torch.float64, device=DEV)
        check(lib.cfen_image_msssim(1, ptr(ta), ptr(tb), B, 3, H, W, 0.0, 1.0, ptr(scratch), ptr(out), current_stream()), "image_msssim")
        outs.append(out)
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
    sse, levels = ops.image_msssim(ta, tb)
    assert torch.equal(outs[0][:, 0], sse) and torch.equal(outs[0][:, 1:].reshape(B, 5, 2), levels)


def test_refusals():
    z = torch.zeros(1, 175, 300, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(CfenError, match="176"):
        ops.image_msssim(z, z)
    with pytest.raises(CfenError, match="176"):
        ops.image_msssim(z.permute(0, 2, 1, 3).contiguous(), z.permute(0, 2, 1, 3).contiguous())
    with pytest.raises(ValueError, match="differ"):
        ops.image_msssim(torch.zeros(1, 176, 176, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 176, 177, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.image_msssim(torch.zeros(1, 2, 176, 176, device=DEV), torch.zeros(1, 2, 176, 176, device=DEV))
    z = torch.zeros(176, 176, 3, dtype=torch.uint8, device=DEV)
    sse, levels = ops.image_msssim(z, z)
    assert sse.tolist() == [0.0] and levels.shape == (1, 5, 2) and (levels == 1.0).all()


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
TINY = NetConfig(24, 4, patch_size=8, load_size=64)            # T = 128


def _run_cli(tmp_path, data, name, extra, tag):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--dataroot", str(data), "--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4",
           "--sb", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--results_dir", str(tmp_path / ("res_" + tag)), "--out_all"] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)


def _dataset(root, size, seed):
    from PIL import Image
    rs = np.random.RandomState(seed)
    os.makedirs(root / "hazy")
    os.makedirs(root / "clear")
    H, W = size
    pairs = {"scene.png": "scene.png", "1400_1.png": "1400.png"}
    for hazy, clear in pairs.items():
        # blocks of 8 plus noise, and a veiled copy: positively correlated at every level, so that MS-SSIM is a number
        img = np.clip(mi._image(rs, H, W, 8) + rs.randint(-12, 13, (H, W, 3)), 0, 255)
        Image.fromarray(img.astype(np.uint8)).save(root / "clear" / clear)
        Image.fromarray(np.clip(img * 3 // 4 + 40 + rs.randint(-6, 7, (H, W, 3)), 0, 255).astype(np.uint8)).save(root / "hazy" / hazy)
    return pairs


def test_cli_eval_metrics_adds_the_msssim_column_and_changes_nothing_else(tmp_path, fixture):
    from PIL import Image
    d_ms = float(fixture["D_ms"])
    name = "iid_hlgvit_crs_gd4_cfs_v3_eval"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    data = tmp_path / "data"
    pairs = _dataset(data, (180, 240), seed=5)
    extra = ["--tile", "--tile_overlap", "16", "--eval"]
    r = _run_cli(tmp_path, data, name, extra + ["--eval_metrics", "psnr,ssim,msssim"], "ms")
    assert r.returncode == 0, r.stdout[-3000:]
    assert "mean PSNR" in r.stdout and "mean SSIM" in r.stdout and "mean MS-SSIM" in r.stdout
    res = tmp_path / "res_ms" / name / "test_32"
    lines = open(res / "metrics.csv").read().splitlines()
    assert lines[0] == "image,psnr,ssim,msssim" and [l.split(",")[0] for l in lines[1:]] == sorted(pairs)
    for line in lines[1:]:
        image, p, s, m = line.split(",")
        out = np.asarray(Image.open(res / "images" / (os.path.splitext(image)[0] + "_fake_A.png")).convert("RGB"))
        gt = np.asarray(Image.open(data / "clear" / pairs[image]).convert("RGB"))
        want = mr.combine(mr.levels_f64_u8(out, gt))
        print("%s: csv msssim %s, float64 from the files: %.9f" % (image, m, want))
        if math.isnan(want):
            assert m == "nan"                                                             # (a seeded net's output may be anticorrelated with the truth)
        else:
            assert abs(float(m) - want) <= 2 * d_ms + 0.5e-6                              # (+ the csv's own %.6f rounding)
    # the same command without --eval_metrics: the same PNG bytes, and the three-column csv it always wrote, equal to the first three columns
    r = _run_cli(tmp_path, data, name, extra, "plain")
    assert r.returncode == 0, r.stdout[-3000:]
    assert "mean SSIM" in r.stdout and "MS-SSIM" not in r.stdout
    assert "eval_metrics" not in [line.split(":")[0] for line in r.stdout.splitlines()]          # the option list it always printed
    ref = tmp_path / "res_plain" / name / "test_32"
    plain = open(ref / "metrics.csv").read().splitlines()
    assert plain[0] == "image,psnr,ssim" and plain[1:] == [l.rsplit(",", 1)[0] for l in lines[1:]]
    files = sorted(os.listdir(res / "images"))
    assert files == sorted(os.listdir(ref / "images")) and len(files) == 2
    for f in files:
        assert open(res / "images" / f, "rb").read() == open(ref / "images" / f, "rb").read(), f


def test_cli_names_an_image_under_176_before_a_checkpoint_is_looked_for(tmp_path):
    name = "iid_hlgvit_crs_gd4_cfs_v3_eval"
    os.makedirs(tmp_path / "ckpt" / name)
    data = tmp_path / "data"
    _dataset(data, (128, 128), seed=6)
    r = _run_cli(tmp_path, data, name, ["--tile", "--tile_overlap", "16", "--eval", "--eval_metrics", "psnr,ssim,msssim"], "ms")     # (no checkpoint written)
    assert r.returncode != 0 and "176" in r.stdout and "1400_1.png" in r.stdout and "128 x 128" in r.stdout
