"""Overlapping-tile inference on the device (cfen_tile_gather / cfen_tile_blend, tiled.dehaze_tiled, test.py --tile) against the float64
restatement in tiling_ref.py and against the plain forward."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import ops, tiled
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict
from cfen_vit_dehazing_amd.util import util
import tiling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY = NetConfig(24, 4, patch_size=8, load_size=64)            # T = 128
FULL512 = NetConfig(24, 4, patch_size=32, load_size=256)       # T = 512
_SD = {}


def make_net(cfg, dtype):
    key = repr(cfg)
    if key not in _SD:
        _SD.clear()
        _SD[key] = generate_state_dict(cfg, seed=0)
    net = dec_ipt(cfg, compute_dtype=dtype)
    net.load_state_dict(_SD[key], strict=True)
    return net.to(DEV)


def random_image(H, W, seed, u8):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (H, W, 3), dtype=np.uint8)
    if u8:
        return a, torch.from_numpy(a).to(DEV)
    f = ((a.astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(2, 0, 1).copy()
    return f, torch.from_numpy(f).to(DEV)


# ---- 1. gather ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("T", [128, 512])
def test_gather_is_the_mirror_index_copy(u8, T):
    o = T // 8
    for k, (H, W) in enumerate([(1, 1), (5, 300), (127, 129), (460, 620), (2160, 3840)]):
        a, img = random_image(H, W, k, u8)
        want = ref.gather(a, T, o, hwc=u8)
        ny, nx = ref.n_tiles(H, T, o), ref.n_tiles(W, T, o)
        n = ny * nx
        assert want.shape[0] == n
        B = 8 if T == 128 else 3
        got = []
        for t0 in range(0, n, B):
            slab = ops.tile_gather(img, T, ny, nx, t0, B)
            got.append(slab.cpu().numpy())
        got = np.concatenate(got)
        assert np.array_equal(got[:n], want), (H, W)
        assert all(np.array_equal(got[t], want[n - 1]) for t in range(n, got.shape[0]))      # padded slots repeat the last tile


# ---- 2. blend ----------------------------------------------------------------------------------------------------------------------------
def _blend_case(H, W, T, o, dtype, B, seed):
    ny, nx = ref.n_tiles(H, T, o), ref.n_tiles(W, T, o)
    n = ny * nx
    nslabs = -(-n // B)
    g = torch.Generator().manual_seed(seed)
    arena = (torch.rand(nslabs * 7 * B * T * T, generator=g) * 2 - 1).to(dtype)
    # the arena's tiles in row-major order as (n, 7, T, T): slab s = [xr (B,3) | xs (B,1) | xd (B,3)]
    tiles = []
    a = arena.double().numpy().reshape(nslabs, 7 * B, T, T)
    for t in range(n):
        s, b = divmod(t, B)
        tiles.append(np.concatenate([a[s, 3 * b:3 * b + 3], a[s, 3 * B + b:3 * B + b + 1], a[s, 4 * B + 3 * b:4 * B + 3 * b + 3]]))
    want, cnt = ref.blend(np.stack(tiles), H, W, T, o)
    return arena.to(DEV), ny, nx, want, cnt


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("o_kind", ["zero", "16", "default", "half"])
def test_blend_matches_float64_reference(dtype, o_kind):
    for H, W, T, B, seed in [(300, 200, 128, 4, 1), (70, 45, 128, 8, 2), (460, 620, 128, 5, 3), (129, 383, 128, 2, 4), (600, 1100, 512, 3, 5)]:
        o = {"zero": 0, "16": 16, "default": T // 8, "half": T // 2}[o_kind]
        arena, ny, nx, want, cnt = _blend_case(H, W, T, o, dtype, B, seed)
        xr, xs, xd = ops.tile_blend(arena, B, T, H, W, ny, nx, o)
        got = torch.cat([xr, xs, xd]).cpu().numpy()
        assert got.shape == (7, H, W)
        assert np.abs(got - want).max() <= 2e-6, (H, W, T, o)
        single = cnt == 1
        assert np.array_equal(got[:, single], want[:, single].astype(np.float32))          # one covering tile: its value, bitwise
        u8 = ops.tile_blend(arena, B, T, H, W, ny, nx, o, output_u8=True)
        for img, plane in zip(u8, (xr, xs, xd)):
            assert np.array_equal(img.cpu().numpy(), util.tensor2im(plane.cpu()))
        again = ops.tile_blend(arena, B, T, H, W, ny, nx, o)
        assert all(torch.equal(p, q) for p, q in zip((xr, xs, xd), again))                  # run-to-run bitwise
        again8 = ops.tile_blend(arena, B, T, H, W, ny, nx, o, output_u8=True)
        assert all(torch.equal(p, q) for p, q in zip(u8, again8))


def test_blend_refuses_a_short_arena():
    arena = torch.zeros(7 * 128 * 128, device=DEV)
    with pytest.raises(ValueError):
        ops.tile_blend(arena, 1, 128, 300, 200, 3, 2, 16)


# ---- 3. one tile: the plain forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [TINY, FULL512], ids=["tiny", "full512"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_single_tile_is_the_plain_forward(cfg, dtype):
    net = make_net(cfg, dtype)
    T = cfg.image_size
    for u8_in in (False, True):
        _, img = random_image(T, T, 7, u8_in)
        plain = [t.clone() for t in net(img[None])]
        got = net.forward_tiled(img)
        for p, g in zip(plain, got):
            assert p.shape[1:] == g.shape and torch.equal(p[0], g)
        net.output_u8 = True
        plain8 = [t.clone() for t in net(img[None])]
        net.output_u8 = False
        got8 = net.forward_tiled(img[None], output_u8=True)
        for p, g in zip(plain8, got8):
            assert p.shape == g.shape and torch.equal(p, g)
        assert net.output_u8 is False


# ---- 4. many tiles: the blend of plain forwards ------------------------------------------------------------------------------------------
def _tiled_reference(net, a, u8, T, o, tile_batch):
    """numpy gather -> the plain forward on the same batches of tiles (the last one padded with the last tile) -> float64 blend"""
    tiles = ref.gather(a, T, o, hwc=u8)
    n = tiles.shape[0]
    B = min(tile_batch, n)
    outs = []
    for t0 in range(0, n, B):
        idx = [min(t, n - 1) for t in range(t0, t0 + B)]
        x = torch.from_numpy(np.ascontiguousarray(tiles[idx])).to(DEV)
        xr, xs, xd = net(x)
        outs.append(torch.cat([xr, xs, xd], 1).double().cpu().numpy())
    H, W = (a.shape[0], a.shape[1]) if u8 else (a.shape[1], a.shape[2])
    return ref.blend(np.concatenate(outs)[:n], H, W, T, o)[0]


@pytest.mark.parametrize("case", ["tiny_300x200_f32", "tiny_70x45_u8", "tiny_200x300_u8_fp16", "full512_fp16_1080x1920"])
def test_tiled_equals_blend_of_plain_forwards(case):
    cfg, dtype, H, W, u8, o = {"tiny_300x200_f32": (TINY, "fp32", 300, 200, False, 16),
                               "tiny_70x45_u8": (TINY, "fp32", 70, 45, True, 16),
                               "tiny_200x300_u8_fp16": (TINY, "fp16", 200, 300, True, None),
                               "full512_fp16_1080x1920": (FULL512, "fp16", 1080, 1920, True, None)}[case]
    net = make_net(cfg, dtype)
    T = cfg.image_size
    a, img = random_image(H, W, 11, u8)
    got = torch.cat(net.forward_tiled(img, overlap=o, tile_batch=4)).cpu().numpy()
    want = _tiled_reference(net, a, u8, T, tiled.default_overlap(T) if o is None else o, 4)
    assert got.shape == (7, H, W)
    err = np.abs(got - want).max()
    print("%s: tiled vs blend of plain forwards max-abs %.2e" % (case, err))
    assert err <= 1e-5


def test_tiled_initialises_pending_actnorm_from_the_first_tile_batch():
    from cfen_vit_dehazing_amd.manifest import generate_state_dict as gen
    sd = gen(TINY, seed=0, mode="reference_init")
    a, img = random_image(200, 150, 3, False)
    net = dec_ipt(TINY, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    net.to(DEV)
    assert any(int(b) == 0 for k, b in net.named_buffers() if k.endswith("initialized"))
    got = torch.cat(net.forward_tiled(img, tile_batch=2)).cpu().numpy()
    assert all(int(b) != 0 for k, b in net.named_buffers() if k.endswith("initialized"))
    # a second net initialised by a plain forward of the same first tile batch computes the same
    ref_net = dec_ipt(TINY, compute_dtype="fp32")
    ref_net.load_state_dict(sd, strict=True)
    ref_net.to(DEV)
    tiles = ref.gather(a, 128, 16, hwc=False)
    ref_net(torch.from_numpy(np.ascontiguousarray(tiles[:2])).to(DEV))
    want = _tiled_reference(ref_net, a, False, 128, 16, 2)
    assert np.abs(got - want).max() <= 1e-5


def test_arena_limit_names_the_image_size():
    net = make_net(TINY, "fp32")
    img = torch.zeros(3, 1000, 900, device=DEV)
    with pytest.raises(ValueError, match="1000 x 900"):
        net.forward_tiled(img, max_arena_bytes=1 << 20)
    with pytest.raises(RuntimeError):
        net(img[None])                                       # the plain forward still refuses other sizes


# ---- 5. CLI ------------------------------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, data, name, extra, check=True):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "test.py"), "--dataroot", str(data), "--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4",
           "--sb", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--results_dir", str(tmp_path / ("res_" + data.name))] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)


@pytest.mark.parametrize("u8_input", [False, True])
def test_cli_tile_writes_input_sized_pngs(tmp_path, u8_input):
    from PIL import Image
    name = "iid_hlgvit_crs_gd4_cfs_v3_tiled"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    rs = np.random.RandomState(0)
    big = rs.randint(0, 256, (200, 300, 3), dtype=np.uint8)
    small = rs.randint(0, 256, (128, 128, 3), dtype=np.uint8)
    for d, imgs in (("both", {"big": big, "small": small}), ("plain", {"small": small})):
        os.makedirs(tmp_path / d / "hazy")
        for stem, a in imgs.items():
            Image.fromarray(a).save(tmp_path / d / "hazy" / (stem + ".png"))
    extra = ["--out_all"] + (["--u8_input"] if u8_input else [])
    r = _run_cli(tmp_path, tmp_path / "both", name, extra + ["--tile", "--tile_overlap", "16"])
    assert r.returncode == 0, r.stdout[-3000:]
    out = tmp_path / "res_both" / name / "test_32" / "images"
    assert sorted(os.listdir(out)) == ["big_fake_A.png", "small_fake_A.png"]
    assert np.asarray(Image.open(out / "big_fake_A.png")).shape == (200, 300, 3)
    r = _run_cli(tmp_path, tmp_path / "plain", name, extra)
    assert r.returncode == 0, r.stdout[-3000:]
    plain = tmp_path / "res_plain" / name / "test_32" / "images" / "small_fake_A.png"
    assert np.array_equal(np.asarray(Image.open(out / "small_fake_A.png")), np.asarray(Image.open(plain)))
    if not u8_input:
        r = _run_cli(tmp_path, tmp_path / "both", name, extra + ["--tile", "--batchSize", "2"])
        assert r.returncode != 0 and "--tile" in r.stdout and "--batchSize 1" in r.stdout
