"""Self-ensemble (x8) on the device (cfen_x8_expand / cfen_x8_merge, ensemble.dehaze_x8, dec_ipt.forward_x8, test.py --self_ensemble) against
the float64 restatement in ensemble_ref.py and against the explicit composition written with torch ops and the plain forward."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import ops
from cfen_vit_dehazing_amd._lib import CfenError
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict
from cfen_vit_dehazing_amd.util import util
import ensemble_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TINY = NetConfig(24, 4, patch_size=8, load_size=64)            # T = 128
FULL512 = NetConfig(24, 4, patch_size=32, load_size=256)       # T = 512
# seven fp32 adds with partial sums <= 8 in magnitude (values in [-1, 1]), then the exact 1/8
BAR = 7 * 2.0 ** -24
_SD = {}


def make_net(cfg, dtype):
    key = repr(cfg)
    if key not in _SD:
        _SD.clear()
        _SD[key] = generate_state_dict(cfg, seed=0)
    net = dec_ipt(cfg, compute_dtype=dtype)
    net.load_state_dict(_SD[key], strict=True)
    return net.to(DEV)


def random_images(M, T, seed, u8):
    a = np.random.RandomState(seed).randint(0, 256, (M, T, T, 3), dtype=np.uint8)
    if u8:
        return a, torch.from_numpy(a).to(DEV)
    f = np.ascontiguousarray(((a.astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(0, 3, 1, 2))
    return f, torch.from_numpy(f).to(DEV)


def t_variant(x, i, hwc=False):
    """x_i of a torch tensor whose image axes are the last two (or, hwc, the two before the last)"""
    H, W = (-3, -2) if hwc else (-2, -1)
    if i & 1:
        x = torch.flip(x, [W])
    if i & 2:
        x = torch.flip(x, [H])
    if i & 4:
        x = x.transpose(H, W)
    return x.contiguous()


def t_back(y, i):
    if i & 4:
        y = y.transpose(-2, -1)
    if i & 2:
        y = torch.flip(y, [-2])
    if i & 1:
        y = torch.flip(y, [-1])
    return y.contiguous()


def t_merge(ys):
    """the ordered fp32 sum of the eight outputs mapped back, times 1/8, with torch ops"""
    acc = t_back(ys[0].float(), 0)
    for i in range(1, 8):
        acc = acc + t_back(ys[i].float(), i)
    return acc * 0.125


def composition(net, images, u8):
    """forward_x8 spelled out: torch flips / transposes, the plain forward of the batch of eight, torch inverse transforms, ordered sum"""
    outs = []
    for m in range(images.shape[0]):
        batch = torch.stack([t_variant(images[m], i, hwc=u8) for i in range(8)])
        ys = [t.clone() for t in net(batch)]
        outs.append([t_merge([y[i] for i in range(8)]) for y in ys])
    return [torch.stack([o[k] for o in outs]) for k in range(3)]


# ---- 1. expand -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("T", [128, 512, 48])
def test_expand_is_the_index_copy(u8, T):
    a, img = random_images(3, T, T, u8)
    for m in range(3):
        got = ops.x8_expand(img, m)
        ax = a[m].transpose(2, 0, 1) if u8 else a[m]                      # (3,T,T) planes for the restatement
        want = ref.variants(ax)
        want = np.ascontiguousarray(want.transpose(0, 2, 3, 1)) if u8 else want
        assert got.shape == want.shape and np.array_equal(got.cpu().numpy(), want), (T, m)
        for i in range(8):
            assert torch.equal(got[i], t_variant(img[m], i, hwc=u8))


# ---- 2. merge ------------------------------------------------------------------------------------------------------------------------------
def _arena(M, T, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(M * 56 * T * T, generator=g) * 2 - 1).to(dtype)


def _arena_outputs(arena, M, T):
    """[(M,8,3,T,T), (M,8,1,T,T), (M,8,3,T,T)] views of the slabs [xr (8,3) | xs (8,1) | xd (8,3)]"""
    a = arena.view(M, 56, T, T)
    return a[:, :24].reshape(M, 8, 3, T, T), a[:, 24:32].reshape(M, 8, 1, T, T), a[:, 32:].reshape(M, 8, 3, T, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M,T", [(1, 128), (3, 128), (2, 512), (2, 48), (1, 16)])
def test_merge_matches_float64_and_the_ordered_torch_sum(dtype, M, T):
    host = _arena(M, T, dtype, 7 * M + T)
    arena = host.to(DEV)
    got = ops.x8_merge(arena, M, T)
    assert [tuple(t.shape) for t in got] == [(M, 3, T, T), (M, 1, T, T), (M, 3, T, T)] and all(t.dtype == torch.float32 for t in got)
    worst = 0.0
    for g, ys_h, ys_d in zip(got, _arena_outputs(host, M, T), _arena_outputs(arena, M, T)):
        want64 = np.stack([ref.merge(ys_h[m].double().numpy()) for m in range(M)])
        worst = max(worst, float(np.abs(g.cpu().numpy().astype(np.float64) - want64).max()))
        want32 = torch.stack([t_merge([ys_d[m, i] for i in range(8)]) for m in range(M)])
        assert torch.equal(g, want32)                                      # the same sequential sum with torch ops on the device: bitwise
    print("merge %s M %d T %d: max |device - float64| %.3e (bar %.3e)" % (dtype, M, T, worst, BAR))
    assert worst <= BAR
    u8 = ops.x8_merge(arena, M, T, output_u8=True)
    for img, plane in zip(u8, got):
        assert tuple(img.shape) == (M, T, T, 3) and img.dtype == torch.uint8
        for m in range(M):
            assert np.array_equal(img[m].cpu().numpy(), util.tensor2im(plane[m].cpu()))
            assert torch.equal(img[m], ops.tensor2im_u8(plane[m].contiguous()))
    flat = torch.empty(7 * M * T * T, dtype=torch.float32, device=DEV)
    views = ops.x8_merge(arena, M, T, out=flat)
    assert all(torch.equal(p, q) for p, q in zip(views, got)) and views[0].data_ptr() == flat.data_ptr()
    assert torch.equal(flat, torch.cat([t.reshape(-1) for t in got]))


def test_merge_slabs_are_independent_repeatable_and_stream_safe():
    M, T = 3, 128
    for dtype in (torch.float32, torch.float16):
        arena = _arena(M, T, dtype, 5).to(DEV)
        both = [ops.x8_merge(arena, M, T), ops.x8_merge(arena, M, T, output_u8=True)]
        for u8, outs in enumerate(both):
            for m in range(M):
                one = ops.x8_merge(arena[m * 56 * T * T:(m + 1) * 56 * T * T], 1, T, output_u8=bool(u8))
                assert all(torch.equal(o[m], p[0]) for o, p in zip(outs, one))
            again = ops.x8_merge(arena, M, T, output_u8=bool(u8))
            assert all(torch.equal(p, q) for p, q in zip(outs, again))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                other = ops.x8_merge(arena, M, T, output_u8=bool(u8))
            side.synchronize()
            assert all(torch.equal(p, q) for p, q in zip(outs, other))


def test_ops_refuse_bad_shapes():
    with pytest.raises(ValueError):
        ops.x8_merge(torch.zeros(56 * 128 * 128 - 1, device=DEV), 1, 128)
    with pytest.raises(ValueError):
        ops.x8_expand(torch.zeros(1, 3, 128, 64, device=DEV))
    with pytest.raises(CfenError, match="multiple of 16"):
        ops.x8_expand(torch.zeros(1, 3, 40, 40, device=DEV))
    with pytest.raises(CfenError, match="image 2"):
        ops.x8_expand(torch.zeros(2, 3, 32, 32, device=DEV), 2)


# ---- 3. forward_x8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [TINY, FULL512], ids=["tiny", "full512"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_forward_x8_is_the_explicit_composition(cfg, dtype):
    net = make_net(cfg, dtype)
    T = cfg.image_size
    M = 2 if cfg is TINY else 1
    for u8_in in (False, True):
        _, img = random_images(M, T, 21, u8_in)
        want = composition(net, img, u8_in)
        got = net.forward_x8(img)
        assert [tuple(t.shape) for t in got] == [(M, 3, T, T), (M, 1, T, T), (M, 3, T, T)]
        for w, g in zip(want, got):
            assert torch.equal(w, g)
        got8 = net.forward_x8(img, output_u8=True)
        for g8, g in zip(got8, got):
            assert torch.equal(g8, torch.stack([ops.tensor2im_u8(g[m].contiguous()) for m in range(M)]))
        assert net.output_u8 is False
    # the eight forwards really differ (the generator is not equivariant): the ensemble is not the plain forward
    plain = net(img)
    assert float((plain[2] - got[2]).abs().max()) > 1e-4


def test_forward_x8_reads_an_fp16_arena_of_an_output_f16_net():
    net = make_net(FULL512, "fp16")
    _, img = random_images(1, 512, 22, True)
    net.output_f16 = True
    want = composition(net, img, True)              # the plain forward's fp16 outputs, widened, mapped back, summed in order
    got = net.forward_x8(img)
    net.output_f16 = False
    assert all(g.dtype == torch.float32 and torch.equal(w, g) for w, g in zip(want, got))


def test_forward_x8_batches_repeats_and_streams_are_bitwise():
    net = make_net(TINY, "fp32")
    _, img = random_images(3, 128, 23, False)
    got = net.forward_x8(img)
    for m in range(3):
        one = net.forward_x8(img[m:m + 1])
        assert all(torch.equal(g[m], o[0]) for g, o in zip(got, one))
    again = net.forward_x8(img)
    assert all(torch.equal(p, q) for p, q in zip(got, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = net.forward_x8(img)
    side.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(got, other))
    flat = torch.empty(7 * 3 * 128 * 128, dtype=torch.float32, device=DEV)
    views = net.forward_x8(img, out=flat)
    assert all(torch.equal(p, q) for p, q in zip(got, views)) and views[0].data_ptr() == flat.data_ptr()


def test_forward_x8_refuses_other_sizes_and_uninitialised_actnorm():
    net = make_net(TINY, "fp32")
    with pytest.raises(ValueError, match="128"):
        net.forward_x8(torch.zeros(1, 3, 256, 256, device=DEV))
    with pytest.raises(ValueError):
        net.forward_x8(torch.zeros(3, 128, 128, device=DEV))
    raw = dec_ipt(TINY, compute_dtype="fp32")
    raw.load_state_dict(generate_state_dict(TINY, seed=0, mode="reference_init"), strict=True)
    raw.to(DEV)
    _, img = random_images(1, 128, 24, False)
    with pytest.raises(CfenError, match="ActNorm"):
        raw.forward_x8(img)
    with pytest.raises(CfenError, match="ActNorm"):
        raw.forward_tiled(img[0], self_ensemble=True)
    raw(img)                                         # one plain forward initialises them
    assert all(torch.isfinite(t).all() for t in raw.forward_x8(img))


# ---- 4. tiled with the ensemble ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_tiled_ensemble_on_one_tile_is_forward_x8(dtype):
    net = make_net(TINY, dtype)
    for u8_in in (False, True):
        _, img = random_images(1, 128, 25, u8_in)
        want = net.forward_x8(img)
        got = net.forward_tiled(img[0], self_ensemble=True)
        assert all(torch.equal(w[0], g) for w, g in zip(want, got))
        want8 = net.forward_x8(img, output_u8=True)
        got8 = net.forward_tiled(img, output_u8=True, self_ensemble=True)
        assert all(torch.equal(w, g) for w, g in zip(want8, got8))


def test_tiled_ensemble_on_many_tiles_is_the_blend_of_forward_x8_tiles():
    import tiling_ref
    net = make_net(TINY, "fp32")
    H, W, T, o = 200, 300, 128, 16
    a = np.random.RandomState(26).randint(0, 256, (H, W, 3), dtype=np.uint8)
    got = torch.cat(net.forward_tiled(torch.from_numpy(a).to(DEV), overlap=o, tile_batch=4, self_ensemble=True)).cpu().numpy()
    tiles = tiling_ref.gather(a, T, o, hwc=True)
    n = tiles.shape[0]
    outs = []
    for t0 in range(0, n, 4):
        idx = [min(t, n - 1) for t in range(t0, t0 + 4)]
        xr, xs, xd = net.forward_x8(torch.from_numpy(np.ascontiguousarray(tiles[idx])).to(DEV))
        outs.append(torch.cat([xr, xs, xd], 1).double().cpu().numpy())
    want = tiling_ref.blend(np.concatenate(outs)[:n], H, W, T, o)[0]
    assert got.shape == (7, H, W) and np.abs(got - want).max() <= 1e-5


# ---- 5. the ensemble commutes with the eight transforms, up to what the plain forward itself varies by ----------------------------------------
def test_forward_x8_commutes_with_the_transforms():
    net = make_net(TINY, "fp32")
    _, img = random_images(1, 128, 27, False)
    # what the PLAIN forward shows for one image at two batch positions: the batch of the eight variants, rolled through all eight positions
    batch = torch.stack([t_variant(img[0], i) for i in range(8)])
    base = [t.clone() for t in net(batch)]
    position = 0.0
    for s in range(1, 8):
        rolled = net(torch.roll(batch, s, 0))
        position = max(position, max(float((torch.roll(r, -s, 0) - b).abs().max()) for r, b in zip(rolled, base)))
    bar = 2 * BAR + position
    want = net.forward_x8(img)
    worst = 0.0
    for g in range(8):
        got = net.forward_x8(t_variant(img, g))
        worst = max(worst, max(float((t_variant(w, g) - o).abs().max()) for w, o in zip(want, got)))
    print("forward_x8(g(x)) against g(forward_x8(x)): worst %.3e, bar %.3e (plain forward at two batch positions: %.3e)" % (worst, bar, position))
    assert worst <= bar


# ---- 6. CLI --------------------------------------------------------------------------------------------------------------------------------
def _run_cli(tmp_path, data, name, extra):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "test.py"), "--dataroot", str(data), "--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4",
           "--sb", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--results_dir", str(tmp_path / ("res_" + data.name))] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)


def test_cli_self_ensemble_writes_the_pngs_of_forward_x8(tmp_path):
    from PIL import Image
    name = "iid_hlgvit_crs_gd4_cfs_v3_x8"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    rs = np.random.RandomState(1)
    imgs = {"a_1": rs.randint(0, 256, (128, 128, 3), dtype=np.uint8), "b_1": rs.randint(0, 256, (128, 128, 3), dtype=np.uint8),
            "c_1": rs.randint(0, 256, (128, 128, 3), dtype=np.uint8)}
    for d in ("alone", "combo", "plain"):
        os.makedirs(tmp_path / d / "hazy")
        os.makedirs(tmp_path / d / "clear")
        for stem, a in imgs.items():
            Image.fromarray(a).save(tmp_path / d / "hazy" / (stem + ".png"))
            Image.fromarray(255 - a).save(tmp_path / d / "clear" / (stem.split("_")[0] + ".png"))
    net = make_net(TINY, "fp32")
    stack = torch.from_numpy(np.stack([imgs[k] for k in sorted(imgs)])).to(DEV)
    # the dataset's own ToTensor + Normalize, on the host as the loader runs it (a device tensor divided by a Python scalar is multiplied by the
    # rounded reciprocal instead: another float in the last place)
    from cfen_vit_dehazing_amd.data import to_normalized_tensor
    x = torch.stack([to_normalized_tensor(imgs[k]) for k in sorted(imgs)]).to(DEV)
    want = [t.cpu().numpy() for t in net.forward_x8(x.contiguous(), output_u8=True)]
    want_u8in = [t.cpu().numpy() for t in net.forward_x8(stack, output_u8=True)]           # --u8_input: the generator normalises the bytes itself
    labels = {"fake_R": 0, "fake_S": 1, "fake_A": 2}

    # alone, all visuals, two images per batch (the last batch holds one)
    r = _run_cli(tmp_path, tmp_path / "alone", name, ["--self_ensemble", "--batchSize", "2"])
    assert r.returncode == 0, r.stdout[-3000:]
    out = tmp_path / "res_alone" / name / "test_32" / "images"
    for k, stem in enumerate(sorted(imgs)):
        for lab, j in labels.items():
            assert np.array_equal(np.asarray(Image.open(out / ("%s_%s.png" % (stem, lab)))), want[j][k]), (stem, lab)
    # with --tile --eval --gpu_png --out_all --u8_input (one tile per image: the blend passes forward_x8's values through)
    r = _run_cli(tmp_path, tmp_path / "combo", name, ["--self_ensemble", "--tile", "--eval", "--gpu_png", "--out_all", "--u8_input"])
    assert r.returncode == 0, r.stdout[-3000:]
    out = tmp_path / "res_combo" / name / "test_32"
    assert sorted(os.listdir(out / "images")) == ["%s_fake_A.png" % s for s in sorted(imgs)]
    for k, stem in enumerate(sorted(imgs)):
        assert np.array_equal(np.asarray(Image.open(out / "images" / (stem + "_fake_A.png"))), want_u8in[2][k]), stem
    rows = open(out / "metrics.csv").read().splitlines()
    assert rows[0] == "image,psnr,ssim" and [row.split(",")[0] for row in rows[1:]] == [s + ".png" for s in sorted(imgs)]
    # --precision half says that the guard does not cover the ensemble; the pipelined driver is refused
    r = _run_cli(tmp_path, tmp_path / "plain", name, ["--self_ensemble", "--precision", "half", "--out_all"])
    assert r.returncode == 0 and "guard does not cover" in r.stdout, r.stdout[-3000:]
    r = _run_cli(tmp_path, tmp_path / "plain", name, ["--self_ensemble", "--in_flight", "2"])
    assert r.returncode != 0 and "--self_ensemble" in r.stdout and "--in_flight 1" in r.stdout
    # without the flag: the plain forward's files, which differ from the ensemble's
    r = _run_cli(tmp_path, tmp_path / "plain", name, ["--out_all", "--precision", "single"])
    assert r.returncode == 0, r.stdout[-3000:]
    net.output_u8 = True
    plain = net(x[0:1].contiguous())[2].cpu().numpy()                 # (the CLI runs --batchSize 1 here)
    net.output_u8 = False
    got = np.asarray(Image.open(tmp_path / "res_plain" / name / "test_32" / "images" / "a_1_fake_A.png"))
    assert np.array_equal(got, plain[0]) and not np.array_equal(got, want[2][0])
