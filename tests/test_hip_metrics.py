"""PSNR / SSIM on the device (cfen_image_metrics, ops.image_metrics, metrics.psnr_ssim, test.py --eval) against the reference's
pytorch_msssim values and their float64 restatement (tests/golden/metrics_pairs.npz, tests/metrics_images.py).

Bars.  The reference itself runs in fp32; the fixture stores D = max |ref32 - f64| over its own cases.  The kernel also works in fp32 with another
summation order, so its SSIM must be within 2 D of the float64 value and within 3 D of the reference's.  The squared error of uint8 input is an
integer sum and must be exact.  The worst measured differences go to profiles/metrics_parity.json (CFEN_WRITE_PARITY=1)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import metrics, ops
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import metrics_images as mi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WORST = {}


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "metrics_pairs.npz"))


def _record(mode, name, d64, d32, dist):
    w = _WORST.setdefault(mode, {"worst_abs_diff_from_f64": 0.0, "worst_abs_diff_from_ref32": 0.0, "worst_case": None})
    if d64 >= w["worst_abs_diff_from_f64"]:
        w["worst_abs_diff_from_f64"], w["worst_case"] = d64, name
    w["worst_abs_diff_from_ref32"] = max(w["worst_abs_diff_from_ref32"], d32)
    if os.environ.get("CFEN_WRITE_PARITY") == "1":
        with open(os.path.join(ROOT, "profiles", "metrics_parity.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reference_fp32_distance_D": dist, "bar_f64": 2 * dist, "bar_ref32": 3 * dist,
                       "modes": _WORST}, f, indent=1, sort_keys=True)
            f.write("\n")


def _check(mode, name, fixture, sse, ssim, exact_sse=True, sse_slack=None):
    k = list(mi.CASES).index(name)
    lo, hi = int(fixture["offsets"][k]), int(fixture["offsets"][k + 1])
    dist = float(fixture["max_ref32_f64"])
    sse, ssim = sse.cpu().numpy(), ssim.cpu().numpy()
    assert sse.shape == ssim.shape == (hi - lo,) and sse.dtype == ssim.dtype == np.float64
    for i in range(hi - lo):
        d64, d32 = abs(ssim[i] - fixture["f64"][lo + i]), abs(ssim[i] - fixture["ref32"][lo + i])
        print("%s %s[%d]: ssim %.9f  |-f64| %.3e (bar %.3e)  |-ref32| %.3e (bar %.3e)  sse %.1f (want %d)"
              % (mode, name, i, ssim[i], d64, 2 * dist, d32, 3 * dist, sse[i], fixture["sse"][lo + i]))
        _record(mode, name, float(d64), float(d32), dist)
        assert d64 <= 2 * dist and d32 <= 3 * dist, (mode, name, i)
        want = int(fixture["sse"][lo + i])
        if exact_sse:
            assert sse[i] == float(want) and float(want) == want, (mode, name, i)
        else:
            assert abs(sse[i] - want) <= sse_slack[i], (mode, name, i, sse[i], want, sse_slack[i])


@pytest.mark.parametrize("name", list(mi.CASES))
def test_uint8_pairs_match_the_reference_and_the_integer_error(name, fixture):
    a, b = mi.pair(name)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sse, ssim = ops.image_metrics(ta, tb)
    _check("uint8", name, fixture, sse, ssim)
    n = a[0].size
    rows = metrics.psnr_ssim(ta, tb)
    k = list(mi.CASES).index(name)
    for i, (p, s) in enumerate(rows):
        want = int(fixture["sse"][int(fixture["offsets"][k]) + i])
        if want == 0:
            assert p == float("inf") and s == 1.0
        else:
            assert abs(p - 10.0 * math.log10(255.0 ** 2 * n / want)) <= 1e-9
        assert s == float(ssim[i])


def _sse_slack(a, b, eps01):
    """fp32 input: each value reaches the kernel within eps01 of v / 255 on the [0,1] scale, so a difference d (0..255 scale) is off by at most
    e = 2 * 255 * eps01 and the sum of d^2 by at most sum(2 |d| e + e^2); plus 1e-12 relative for the fp64 accumulation"""
    e = 2 * 255.0 * eps01
    d = np.abs(a.astype(np.float64) - b.astype(np.float64)).reshape(a.shape[0], -1)
    return (2 * e * d.sum(axis=1) + e * e * d.shape[1]) * (1 + 1e-6) + 1e-12 * (d * d).sum(axis=1)


@pytest.mark.parametrize("name", list(mi.CASES))
def test_float_input_gives_the_uint8_result(name, fixture):
    a, b = mi.pair(name)
    # v / 255 in fp32, divided on the host (IEEE division, what the kernel does to bytes; torch's device division by a scalar multiplies by 1 / 255)
    fa = torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)).to(DEV)
    fb = torch.from_numpy(np.ascontiguousarray(b.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)).to(DEV)
    sse, ssim = ops.image_metrics(fa, fb, value_range=(0.0, 1.0))
    u_sse, u_ssim = ops.image_metrics(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV))
    assert torch.equal(ssim, u_ssim)                                  # (v - 0) / 1 is v: the same fp32 values, the same bits
    _check("float32 range (0,1)", name, fixture, sse, ssim, exact_sse=False, sse_slack=_sse_slack(a, b, 2.0 ** -24))
    # [-1,1] data, the generator's float outputs: ToTensor + Normalize(0.5, 0.5) of the bytes; v/255 rounds (2^-25), (x - .5) / .5 rounds (2^-24 on
    # [-1,1] = 2^-25 on [0,1]), the kernel's (v + 1) / 2 is exact up to the subtraction's rounding (2^-24 on [0,2] = 2^-25): under 2^-23 in all
    na, nb = (fa - 0.5) / 0.5, (fb - 0.5) / 0.5
    sse, ssim = ops.image_metrics(na, nb, value_range=(-1.0, 1.0))
    _check("float32 range (-1,1)", name, fixture, sse, ssim, exact_sse=False, sse_slack=_sse_slack(a, b, 2.0 ** -23))
    # one channel: the mean over one plane is that plane's SSIM
    s1, m1 = ops.image_metrics(fa[:, 1:2].contiguous(), fb[:, 1:2].contiguous(), value_range=(0.0, 1.0))
    want = [mi.ssim_f64(fa[i, 1:2].double().cpu().numpy(), fb[i, 1:2].double().cpu().numpy()) for i in range(min(2, a.shape[0]))]
    for i, w in enumerate(want):
        assert abs(float(m1[i]) - w) <= 2 * float(fixture["max_ref32_f64"])


def test_batch_equals_single_calls_and_calls_repeat_bitwise():
    a, b = mi.pair("512x512_batch8")
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    sse, ssim = ops.image_metrics(ta, tb)
    one = [ops.image_metrics(ta[i:i + 1], tb[i:i + 1]) for i in range(8)]
    assert torch.equal(sse, torch.cat([o[0] for o in one])) and torch.equal(ssim, torch.cat([o[1] for o in one]))
    again = ops.image_metrics(ta, tb)
    assert torch.equal(sse, again[0]) and torch.equal(ssim, again[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.image_metrics(ta, tb)
    side.synchronize()
    assert torch.equal(sse, other[0]) and torch.equal(ssim, other[1])
    fa, fb = ta.permute(0, 3, 1, 2).float().contiguous(), tb.permute(0, 3, 1, 2).float().contiguous()
    f1, f2 = ops.image_metrics(fa, fb, value_range=(0.0, 255.0)), ops.image_metrics(fa, fb, value_range=(0.0, 255.0))
    assert torch.equal(f1[0], f2[0]) and torch.equal(f1[1], f2[1])
    assert torch.equal(f1[1], ssim)                                                # v / 255 by the range mapping: the uint8 path's values


def test_python_side_refusals():
    z = torch.zeros(1, 10, 64, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(Exception, match="11 x 11"):
        ops.image_metrics(z, z)
    with pytest.raises(ValueError, match="differ"):
        ops.image_metrics(torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device=DEV), torch.zeros(1, 16, 17, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        ops.image_metrics(torch.zeros(1, 2, 16, 16, device=DEV), torch.zeros(1, 2, 16, 16, device=DEV))
    sse, ssim = ops.image_metrics(torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV), torch.zeros(16, 16, 3, dtype=torch.uint8, device=DEV))
    assert sse.tolist() == [0.0] and ssim.tolist() == [1.0]


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
    for hazy, clear in (("scene.png", "scene.png"), ("1400_1.png", "1400.png"), ("street.png", "street.jpg")):      # same stem, RESIDE prefix, another extension
        Image.fromarray(rs.randint(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "hazy" / hazy)
        Image.fromarray(rs.randint(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "clear" / clear)
    return {"scene.png": "scene.png", "1400_1.png": "1400.png", "street.png": "street.jpg"}


def _check_csv(res, data, pairs, dist):
    from PIL import Image
    lines = open(res / "metrics.csv").read().splitlines()
    assert lines[0] == "image,psnr,ssim" and [l.split(",")[0] for l in lines[1:]] == sorted(pairs)             # dataset order
    for line in lines[1:]:
        image, p, s = line.split(",")
        out = np.asarray(Image.open(res / "images" / (os.path.splitext(image)[0] + "_fake_A.png")).convert("RGB"))
        gt = np.asarray(Image.open(data / "clear" / pairs[image]).convert("RGB"))
        want_p, want_s = mi.psnr_from_sse(mi.sse_int(out, gt), out.size), mi.ssim_f64_u8(out, gt)
        print("%s: csv psnr %s ssim %s, float64 from the files: %.9f %.9f" % (image, p, s, want_p, want_s))
        assert abs(float(p) - want_p) <= 1e-6 and abs(float(s) - want_s) <= 2 * dist + 0.5e-6                  # (+ the csv's own %.6f rounding)


@pytest.mark.parametrize("mode", ["plain_batch2", "tile"])
def test_cli_eval_scores_the_written_pngs(tmp_path, mode, fixture):
    dist = float(fixture["max_ref32_f64"])
    name = "iid_hlgvit_crs_gd4_cfs_v3_eval"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    data = tmp_path / "data"
    pairs = _dataset(data, (128, 128) if mode == "plain_batch2" else (150, 200), seed=3)
    extra = ["--batchSize", "2"] if mode == "plain_batch2" else ["--tile", "--tile_overlap", "16"]
    r = _run_cli(tmp_path, data, name, extra + ["--eval"], "eval")
    assert r.returncode == 0, r.stdout[-3000:]
    assert "mean PSNR" in r.stdout and "mean SSIM" in r.stdout
    res = tmp_path / "res_eval" / name / "test_32"
    _check_csv(res, data, pairs, dist)
    # the same command without --eval: the same PNG bytes, no csv
    r = _run_cli(tmp_path, data, name, extra, "plain")
    assert r.returncode == 0, r.stdout[-3000:]
    ref = tmp_path / "res_plain" / name / "test_32"
    assert not os.path.exists(ref / "metrics.csv") and "mean PSNR" not in r.stdout
    files = sorted(os.listdir(res / "images"))
    assert files == sorted(os.listdir(ref / "images")) and len(files) == 3
    for f in files:
        assert open(res / "images" / f, "rb").read() == open(ref / "images" / f, "rb").read(), f


def test_cli_eval_names_a_missing_ground_truth_before_any_forward(tmp_path):
    name = "iid_hlgvit_crs_gd4_cfs_v3_eval"
    os.makedirs(tmp_path / "ckpt" / name)
    data = tmp_path / "data"
    _dataset(data, (128, 128), seed=4)
    os.remove(data / "clear" / "1400.png")
    r = _run_cli(tmp_path, data, name, ["--eval"], "eval")             # (no checkpoint written: the run must stop before it looks for one)
    assert r.returncode != 0 and "1400_1.png" in r.stdout and "no ground truth" in r.stdout
