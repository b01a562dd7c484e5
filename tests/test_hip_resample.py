"""PIL-exact uint8 resampling on the device (cfen_resample_u8, ops.resample_u8), fit-to-size inference on top of it (dec_ipt.forward_fit,
test.py --fit), and the ledger of include/cfen_resample.h.  The reference of every comparison is Image.resize of the PIL installed here, called
in the test; there is no tolerance anywhere."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from cfen_vit_dehazing_amd import _lib, metrics, ops, resample
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.data import to_normalized_tensor
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import cabi_ledger
import guarded
import resample_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = NetConfig(24, 4, patch_size=8, load_size=64)            # T = 128
T = 128


def images(B, H, W, seed, binary=False):
    rs = np.random.RandomState(seed)
    a = (rs.randint(0, 2, (B, H, W, 3)) * 255).astype(np.uint8) if binary else rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    return a, torch.from_numpy(a).to(DEV)


def pil(a, size, filter="bicubic"):
    return np.stack([ref.pil_resize(x, size, filter) for x in a])


# (B, H, W) -> (H2, W2), filter, 0/255 image: the smallest shapes that reach each path of the two kernels
CASES = {
    "down_2x45x70_32x32": ((2, 45, 70), (32, 32), "bicubic", False),                   # 11 taps staged in LDS; vertical rows of 96 bytes (16-byte vectors)
    "up_32x32_45x70": ((1, 32, 32), (45, 70), "bicubic", False),                       # 5 taps; rows of 210 bytes (byte path)
    "up_128x128_200x300": ((1, 128, 128), (200, 300), "bicubic", False),               # 5 column tiles of 64; rows of 900 bytes (byte path)
    "down_200x300_128x128": ((1, 200, 300), (128, 128), "bicubic", False),
    "horizontal_only": ((1, 64, 50), (64, 32), "bicubic", False),
    "vertical_only": ((1, 50, 64), (32, 64), "bicubic", False),
    "equal_size_is_a_copy": ((2, 50, 64), (50, 64), "bicubic", False),
    "w2_16": ((1, 40, 60), (20, 16), "bicubic", False),                                # 3 W2 % 16 == 0
    "w2_17": ((1, 40, 60), (20, 17), "bicubic", False),                                # 3 W2 % 16 != 0, odd
    "w2_1": ((1, 40, 60), (20, 1), "bicubic", False),
    "h2_1": ((1, 40, 60), (1, 24), "bicubic", False),
    "1x1_5x7": ((1, 1, 1), (5, 7), "bicubic", False),
    "taps_241_and_137": ((1, 540, 960), (16, 16), "bicubic", False),                   # the table that does not fit the staged weights: global path
    "clip_0_255": ((2, 45, 70), (37, 53), "bicubic", True),
    "rows_past_1KiB_vec16": ((1, 20, 24), (30, 400), "bicubic", False),                # rows of 1200 bytes: two segments per row, 16-byte vectors
    "rows_past_1KiB_bytes": ((1, 9, 30), (13, 350), "bicubic", False),                 # rows of 1050 bytes: two segments, byte path, ragged last lane
    "row_blocks_across_images": ((3, 7, 90), (7, 33), "bicubic", False),               # 21 rows: blocks of 4 rows that straddle images, the last one short
    "run_longer_than_the_stage": ((1, 5, 768), (5, 64), "bilinear", False),            # 25 taps fit, the 64 columns' 2304-byte run does not: global path
    "bilinear_down": ((1, 45, 70), (32, 32), "bilinear", False), "bilinear_up": ((1, 32, 32), (45, 70), "bilinear", False),
    "box_down": ((1, 45, 70), (32, 32), "box", False), "box_up": ((1, 32, 32), (45, 70), "box", False),
    "hamming_down": ((1, 45, 70), (32, 32), "hamming", False), "hamming_up": ((1, 32, 32), (45, 70), "hamming", False),
    "lanczos_down": ((1, 45, 70), (32, 32), "lanczos", False), "lanczos_up": ((1, 32, 32), (45, 70), "lanczos", False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_resample_equals_pil(case):
    (B, H, W), size, filter, binary = CASES[case]
    assert filter in resample.FILTERS
    a, t = images(B, H, W, len(case), binary)
    got = ops.resample_u8(t, size, filter)
    assert got.shape == (B,) + size + (3,) and got.dtype == torch.uint8 and got.data_ptr() != t.data_ptr()
    assert np.array_equal(got.cpu().numpy(), pil(a, size, filter)), case


def test_paths_the_cases_claim():
    """the table sizes the cases above rely on to reach the staged and the global path of the horizontal kernel"""
    assert resample.coefficients(70, 32, "bicubic")[1].shape[1] == 11 and resample.coefficients(960, 16, "bicubic")[1].shape[1] == 241
    b, c = resample.coefficients(768, 64, "bilinear")
    assert c.shape[1] == 25 and (int(b[63, 0]) + int(b[63, 1]) - int(b[0, 0])) * 3 > 2048


@pytest.mark.parametrize("size", [(37, 53), (32, 32)])
def test_dst_as_a_lane_of_a_slab(size):
    """out = lane 1 of a (3, H2, W2, 3) slab: at 37 x 53 the lane starts at an odd address (the byte path), at 32 x 32 on a 16-byte boundary; the
    neighbouring lanes keep their bytes"""
    a, t = images(1, 45, 70, 5)
    slab = torch.from_numpy(np.random.RandomState(6).randint(0, 256, (3,) + size + (3,), dtype=np.uint8)).to(DEV)
    before = slab.clone()
    out = ops.resample_u8(t, size, out=slab[1:2])
    assert out.data_ptr() == slab[1].data_ptr() and (out.data_ptr() % 2 == 1) == (size == (37, 53))
    assert np.array_equal(slab[1].cpu().numpy(), pil(a, size)[0])
    assert torch.equal(slab[0], before[0]) and torch.equal(slab[2], before[2])
    with pytest.raises(ValueError, match="resample_u8: out must be"):
        ops.resample_u8(t, size, out=slab[:, :, :, :1])
    with pytest.raises(ValueError, match="resample_u8 needs"):
        ops.resample_u8(t.float(), size)
    with pytest.raises(ValueError, match="unknown resampling filter"):
        ops.resample_u8(t, size, "nearest")


def _raw(t, size, filter, tmp, dst, stream=None):
    """the C entry point with caller-placed tmp and dst"""
    B, H, W, _ = t.shape
    H2, W2 = size
    xb, xc = resample.device_tables(W, W2, filter, t.device)
    yb, yc = resample.device_tables(H, H2, filter, t.device)
    lib = _lib.load()
    _lib.check(lib.cfen_resample_u8(_lib.ptr(t), B, H, W, _lib.ptr(xb), _lib.ptr(xc), xc.shape[1], W2, _lib.ptr(yb), _lib.ptr(yc), yc.shape[1], H2,
                                    _lib.ptr(tmp), _lib.ptr(dst), stream if stream is not None else _lib.current_stream()), "resample_u8")


def test_determinism():
    size = (37, 53)
    a, t = images(3, 45, 70, 9)
    want = pil(a, size)
    whole = ops.resample_u8(t, size)
    assert np.array_equal(whole.cpu().numpy(), want)
    for b in range(3):                                                    # B = 3 equals three B = 1 calls
        assert torch.equal(ops.resample_u8(t[b:b + 1], size), whole[b:b + 1])
    for _ in range(3):                                                    # repeated calls
        assert torch.equal(ops.resample_u8(t, size), whole)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.resample_u8(t, size)
    side.synchronize()
    assert torch.equal(on_side, whole)
    for fill in (0x00, 0xff):                                             # what tmp and dst held before does not matter
        tmp = torch.full((3 * 45 * 53 * 3,), fill, dtype=torch.uint8, device=DEV)
        dst = torch.full((3,) + size + (3,), fill, dtype=torch.uint8, device=DEV)
        _raw(t, size, "bicubic", tmp, dst)
        assert torch.equal(dst, whole)
        assert np.array_equal(tmp.view(3, 45, 53, 3).cpu().numpy(), pil(a, (45, 53)))          # the uint8 intermediate is PIL's horizontal pass


# ---- guard bands and the header's ledger -------------------------------------------------------------------------------------------------
def test_guard_bands_resample_u8():
    """src and the four tables between 0xff bands, tmp and dst prefilled 0xff between random bands: no band changes, every dst byte equals PIL,
    and a zero prefill gives the same bytes"""
    lib = _lib.load()
    B, H, W, H2, W2 = 2, 45, 70, 37, 53
    a, t = images(B, H, W, 21)
    want = pil(a, (H2, W2))
    src = guarded.guarded_copy(t)
    tables = [guarded.guarded_copy(torch.from_numpy(x.copy()), device=DEV) for x in resample.coefficients(W, W2) + resample.coefficients(H, H2)]
    xb, xc, yb, yc = tables
    tmp = guarded.guarded_empty((B * H * W2 * 3,), torch.uint8, DEV, fill="ff")
    dst = guarded.guarded_empty((B, H2, W2, 3), torch.uint8, DEV, fill="ff")
    results = []
    for fill in ("ff", "zero"):
        guarded.refill(tmp, fill)
        guarded.refill(dst, fill)
        _lib.check(lib.cfen_resample_u8(_lib.ptr(src), B, H, W, _lib.ptr(xb), _lib.ptr(xc), xc.shape[1], W2, _lib.ptr(yb), _lib.ptr(yc), yc.shape[1], H2,
                                        _lib.ptr(tmp), _lib.ptr(dst), _lib.current_stream()), "resample_u8")
        torch.cuda.synchronize()
        guarded.check_bands(src, xb, xc, yb, yc, tmp, dst)
        assert np.array_equal(dst.cpu().numpy(), want), fill
        results.append(dst.clone())
    assert torch.equal(results[0], results[1])
    # one pass only, and none: tmp is not touched
    for size in ((H, W2), (H2, W), (H, W)):
        guarded.refill(tmp, "ff")
        one = guarded.guarded_empty((B,) + size + (3,), torch.uint8, DEV, fill="ff")
        hp, vp = size[1] != W, size[0] != H
        _lib.check(lib.cfen_resample_u8(_lib.ptr(src), B, H, W, _lib.ptr(xb if hp else None), _lib.ptr(xc if hp else None), xc.shape[1] if hp else 0,
                                        size[1], _lib.ptr(yb if vp else None), _lib.ptr(yc if vp else None), yc.shape[1] if vp else 0, size[0],
                                        _lib.ptr(tmp), _lib.ptr(one), _lib.current_stream()), "resample_u8")
        torch.cuda.synchronize()
        guarded.check_bands(src, xb, xc, yb, yc, tmp, one)
        assert np.array_equal(one.cpu().numpy(), pil(a, size)), size
        assert bool((guarded.raw_bytes(tmp) == 255).all())


def test_every_function_of_the_resample_header_is_guard_band_tested():
    """what tests/test_cabi.py checks for include/cfen_hip.h, for include/cfen_resample.h: every function it declares is called through lib.
    inside the guard-band test above"""
    fns = cabi_ledger.header_functions("cfen_resample.h")
    assert sorted(fns) == sorted(_lib.HEADERS["cfen_resample.h"])
    cabi_ledger.check_guard_band_test_calls("test_hip_resample.py", "test_guard_bands_resample_u8", fns)


# ---- forward_fit -------------------------------------------------------------------------------------------------------------------------
_SD = {}


def make_net(dtype):
    if "sd" not in _SD:
        _SD["sd"] = generate_state_dict(TINY, seed=0)
    net = dec_ipt(TINY, compute_dtype=dtype)
    net.load_state_dict(_SD["sd"], strict=True)
    return net.to(DEV)


def net_input(a, u8_input):
    """a: (B,T,T,3) uint8 numpy -> what the loader hands the plain forward"""
    if u8_input:
        return torch.from_numpy(a).to(DEV)
    return torch.stack([to_normalized_tensor(Image.fromarray(x)) for x in a]).to(DEV)


def plain_u8(net, x, x8=False):
    if x8:
        return [o.cpu().numpy() for o in net.forward_x8(x, output_u8=True)]
    net.output_u8 = True
    try:
        return [o.clone().cpu().numpy() for o in net(x)]
    finally:
        net.output_u8 = False


@pytest.mark.parametrize("u8_input", [True, False], ids=["u8_input", "float_input"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_forward_fit(dtype, u8_input):
    net = make_net(dtype)
    big, tbig = images(1, 200, 300, 31)
    mid, tmid = images(1, 90, 128, 32)
    same, tsame = images(1, T, T, 33)
    # T x T: the plain forward, bitwise
    want = plain_u8(net, net_input(same, u8_input))
    got = net.forward_fit(tsame, u8_input=u8_input)
    assert all(g.shape == (1, T, T, 3) and g.dtype == torch.uint8 and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))
    assert net.output_u8 is False
    # 200 x 300: PIL resize -> plain forward with uint8 outputs -> PIL resize, all three outputs
    small = pil(big, (T, T))
    want = [pil(o, (200, 300)) for o in plain_u8(net, net_input(small, u8_input))]
    got = net.forward_fit(tbig, u8_input=u8_input)
    for g, w in zip(got, want):
        assert g.shape == (1, 200, 300, 3) and np.array_equal(g.cpu().numpy(), w)
    # the list form: one batch-3 forward
    batch = np.concatenate([small, pil(mid, (T, T)), same])
    outs = plain_u8(net, net_input(batch, u8_input))
    got = net.forward_fit([tbig[0], tmid[0], tsame[0]], u8_input=u8_input)
    assert len(got) == 3 and all(len(g) == 3 for g in got)
    for g, o in zip(got, outs):
        for i, size in enumerate([(200, 300), (90, 128), (T, T)]):
            assert g[i].shape == size + (3,) and np.array_equal(g[i].cpu().numpy(), ref.pil_resize(o[i], size)), (i, size)
    # self-ensemble: forward_x8 of the PIL-resized image, resized back
    want = [pil(o, (200, 300)) for o in plain_u8(net, net_input(small, u8_input), x8=True)]
    got = net.forward_fit(tbig, self_ensemble=True, u8_input=u8_input)
    for g, w in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), w)
    # another filter goes both ways
    want = [pil(o, (200, 300), "bilinear") for o in plain_u8(net, net_input(pil(big, (T, T), "bilinear"), u8_input))]
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(net.forward_fit(tbig, filter="bilinear", u8_input=u8_input), want))
    with pytest.raises(ValueError, match="forward_fit needs"):
        net.forward_fit(tbig.float())


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, data, name, extra):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--dataroot", str(data), "--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4",
           "--sb", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--results_dir", str(tmp_path / ("res_" + data.name))] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)


@pytest.mark.parametrize("u8_input", [False, True])
def test_cli_fit_writes_input_sized_pngs(tmp_path, u8_input):
    name = "iid_hlgvit_crs_gd4_cfs_v3_fit"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    rs = np.random.RandomState(0)
    big = rs.randint(0, 256, (200, 300, 3), dtype=np.uint8)
    small = rs.randint(0, 256, (T, T, 3), dtype=np.uint8)
    gt = {"big": rs.randint(0, 256, (200, 300, 3), dtype=np.uint8), "small": rs.randint(0, 256, (T, T, 3), dtype=np.uint8)}
    for d, imgs in (("both", {"big": big, "small": small}), ("plain", {"big": ref.pil_resize(big, (T, T)), "small": small})):
        os.makedirs(tmp_path / d / "hazy")
        for stem, a in imgs.items():
            Image.fromarray(a).save(tmp_path / d / "hazy" / (stem + ".png"))
    os.makedirs(tmp_path / "both" / "clear")
    for stem, a in gt.items():
        Image.fromarray(a).save(tmp_path / "both" / "clear" / (stem + ".png"))
    extra = ["--out_all"] + (["--u8_input"] if u8_input else [])
    r = _run_cli(tmp_path, tmp_path / "both", name, extra + ["--fit", "--eval"])
    assert r.returncode == 0, r.stdout[-3000:]
    res = tmp_path / "res_both" / name / "test_32"
    assert sorted(os.listdir(res / "images")) == ["big_fake_A.png", "small_fake_A.png"]
    got_big = np.asarray(Image.open(res / "images" / "big_fake_A.png"))
    got_small = np.asarray(Image.open(res / "images" / "small_fake_A.png"))
    assert got_big.shape == (200, 300, 3) and got_small.shape == (T, T, 3)
    # the plain run on the PIL-pre-resized file and on the small one
    r = _run_cli(tmp_path, tmp_path / "plain", name, extra)
    assert r.returncode == 0, r.stdout[-3000:]
    plain = tmp_path / "res_plain" / name / "test_32" / "images"
    assert np.array_equal(got_small, np.asarray(Image.open(plain / "small_fake_A.png")))
    assert np.array_equal(got_big, ref.pil_resize(np.asarray(Image.open(plain / "big_fake_A.png")), (200, 300)))
    # --eval: scored at the original size, the row is metrics.psnr_ssim of the written pixels
    lines = open(res / "metrics.csv").read().splitlines()
    assert lines[0] == "image,psnr,ssim" and [l.split(",")[0] for l in lines[1:]] == ["big.png", "small.png"]
    p, s = metrics.psnr_ssim(torch.from_numpy(got_big.copy())[None].to(DEV), torch.from_numpy(gt["big"])[None].to(DEV))[0]
    assert lines[1] == metrics.format_csv([("big.png", p, s)]).splitlines()[1]
    if not u8_input:
        r = _run_cli(tmp_path, tmp_path / "both", name, extra + ["--fit", "--tile"])
        assert r.returncode != 0 and "--fit" in r.stdout and "--tile" in r.stdout
