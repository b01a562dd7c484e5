"""PNG encoding on the device (cfen_png_deflate, ops.png_deflate, png.encode, test.py --gpu_png) against the numpy restatement of its format
(tests/png_ref.py): the kernels' zlib stream must equal the restatement's byte for byte, PIL must decode the assembled file to the input, and the
bytes must not depend on batch size, call or stream.  The CLI with --gpu_png must write the same file names and the same pixels as without."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import metrics_images as mi
import png_ref
from cfen_vit_dehazing_amd import _lib, ops, png
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.manifest import generate_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = dict(png_ref.SMALL_CASES)
CASES["512x512"] = lambda: mi.pair("512x512_batch8")[0][0]
CASES["2160x3840"] = lambda: png_ref.smooth(2160, 3840, 8)


def _streams(images):
    """list of the device encoder's zlib streams (bytes) of a (B,H,W,3) uint8 numpy array or CUDA tensor"""
    t = images if isinstance(images, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(images)).to(DEV)
    slab, lengths = ops.png_deflate(t)
    slab, lengths = slab.cpu().numpy(), lengths.cpu().numpy()
    return [slab[i, :lengths[i]].tobytes() for i in range(len(lengths))]


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], dtype=np.uint8) != np.frombuffer(b[:n], dtype=np.uint8))[0]
    return "lengths %d / %d, first differing byte %s" % (len(a), len(b), int(d[0]) if len(d) else None)


@pytest.mark.parametrize("name", list(CASES))
def test_stream_equals_the_restatement_and_pil_decodes_the_input(name):
    img = CASES[name]()
    H, W, _ = img.shape
    got = _streams(img[None])[0]
    want = png_ref.stream(img)
    print("%s: %d x %d, stream %d bytes = %.1f %% of raw" % (name, H, W, len(got), 100.0 * len(got) / img.size))
    assert got == want, _first_difference(got, want)
    back = Image.open(io.BytesIO(png.assemble(got, H, W)))
    assert back.mode == "RGB" and back.size == (W, H) and np.array_equal(np.array(back), img)


def test_workspace_geometry_matches_the_python_side():
    lib = _lib.load()
    for B, H, W in ((1, 1, 1), (8, 512, 512), (1, 2160, 3840), (3, 100, 300), (2, 3, 10922)):
        strip, stride = ctypes.c_size_t(0), ctypes.c_size_t(0)
        total = lib.cfen_png_workspace_bytes(B, H, W, ctypes.byref(strip), ctypes.byref(stride))
        R, S, rowb, strip_bytes, out_stride = png.geometry(H, W)
        assert (strip.value, stride.value) == (strip_bytes, out_stride)
        assert total == -(-B * S * 16 // 256) * 256 + B * S * strip_bytes
    assert lib.cfen_png_workspace_bytes(1, 4, 10923, None, None) == 0


def test_batch_calls_and_streams_give_the_same_bytes():
    a, _ = mi.pair("512x512_batch8")
    t = torch.from_numpy(a).to(DEV)
    batch = _streams(t)
    assert len(batch) == 8
    for i in range(8):
        assert _streams(t[i:i + 1].contiguous())[0] == batch[i], i
    assert _streams(t) == batch
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.png_deflate(t)
    side.synchronize()
    assert [other[0][i, :int(other[1][i])].cpu().numpy().tobytes() for i in range(8)] == batch
    assert batch[0] == png_ref.stream(a[0]) and batch[7] == png_ref.stream(a[7])


def test_encode_and_encode_async():
    a, _ = mi.pair("64x64")
    t = torch.from_numpy(np.concatenate([a, a[:, ::-1]])).to(DEV).contiguous()
    files = png.encode(t)
    assert len(files) == 2
    for f, want in zip(files, t.cpu().numpy()):
        assert np.array_equal(np.array(Image.open(io.BytesIO(f))), want)
    pending = png.encode_async(t)
    assert pending.slab.is_pinned() and pending.lengths.is_pinned()
    assert pending.files() == files
    assert png.encode(t[0]) == files[:1]                                   # an image without the batch dimension


def test_row_limit_is_refused_by_the_library_and_falls_back_in_encode():
    wide = torch.from_numpy(png_ref.smooth(2, 10923, 9)).to(DEV)
    with pytest.raises(_lib.CfenError, match="scanline"):
        ops.png_deflate(wide[None].contiguous())
    f = png.encode(wide)                                                   # PIL wrote it
    assert np.array_equal(np.array(Image.open(io.BytesIO(f[0]))), wide.cpu().numpy())
    with pytest.raises(ValueError):
        ops.png_deflate(torch.zeros(1, 3, 8, 8, device=DEV))


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------
TINY = NetConfig(24, 4, patch_size=8, load_size=64)            # T = 128


def _run_cli(tmp_path, data, name, extra, tag):
    cmd = [sys.executable, os.path.join(ROOT, "test.py"), "--dataroot", str(data), "--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4",
           "--sb", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--results_dir", str(tmp_path / ("res_" + tag))] + extra
    return subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=False)


def _dataset(root, size, seed, count):
    rs = np.random.RandomState(seed)
    os.makedirs(root / "hazy")
    H, W = size
    for i in range(count):
        Image.fromarray(png_ref.smooth(H, W, rs.randint(1 << 30))).save(root / "hazy" / ("img%02d.png" % i))


@pytest.mark.parametrize("mode", ["sequential", "in_flight_4", "tile"])
def test_cli_gpu_png_writes_the_same_names_and_pixels(tmp_path, mode):
    name = "iid_hlgvit_crs_gd4_cfs_v3_png"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    data = tmp_path / "data"
    _dataset(data, (150, 200) if mode == "tile" else (128, 128), seed=5, count=3 if mode == "tile" else 9)
    extra = {"sequential": ["--batchSize", "2"],                                        # all four visuals, a ragged last batch
             "in_flight_4": ["--batchSize", "2", "--in_flight", "4", "--writers", "4"],
             "tile": ["--tile", "--tile_overlap", "16", "--out_all"]}[mode]
    r = _run_cli(tmp_path, data, name, extra, "pil")
    assert r.returncode == 0, r.stdout[-3000:]
    r = _run_cli(tmp_path, data, name, extra + ["--gpu_png"], "gpu")
    assert r.returncode == 0, r.stdout[-3000:]
    ref, res = (tmp_path / ("res_" + tag) / name / "test_32" / "images" for tag in ("pil", "gpu"))
    files = sorted(os.listdir(ref))
    assert files == sorted(os.listdir(res)) and len(files) == (3 if mode == "tile" else 36)
    for f in files:
        a, b = Image.open(ref / f), Image.open(res / f)
        assert a.mode == b.mode == "RGB" and a.size == b.size, f
        assert np.array_equal(np.array(a), np.array(b)), f
