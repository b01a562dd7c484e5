"""dehaze_video.py end to end on the TINY net (T = 128): every output frame is, bit for bit, ref.rgb_to_yuv of what the library route returns for
ref.yuv_to_rgb of the input frame with the same batch grouping; the plain and --fit routes are also held against test.py on the same frames as
PNGs.  The conversions both ways are integer (tests/yuv_ref.py) and the forwards are the same launches, so every comparison is bitwise; the
noref.csv values are held to 1e-6 (the %.6f rounding) as in tests/test_hip_noref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import metrics
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import noref_ref
import test_hip_metrics as evalref                     # TINY, _run_cli: the fixtures of the CLI tests
import yuv_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = evalref.ROOT
NAME = "iid_hlgvit_crs_gd4_cfs_v3_video"
T = 128
CASES = {            # route: (frames, H, W, chroma, extra flags)
    "plain": (5, T, T, "420jpeg", ["--batchSize", "2"]),
    "fit": (4, 150, 201, "420mpeg2", ["--fit", "--batchSize", "2"]),
    "tile": (2, 150, 201, "444", ["--tile", "--tile_overlap", "16"]),
}
_NET = []


def _net():
    if not _NET:
        net = dec_ipt(evalref.TINY, compute_dtype="fp32")
        net.load_state_dict(generate_state_dict(evalref.TINY, seed=0), strict=True)
        _NET.append(net)
    return _NET[0]


def _stream(route, seed=11):
    """(the stream's bytes, header, input frames, their RGB by the restatement)"""
    n, H, W, chroma, _ = CASES[route]
    rs = np.random.RandomState(seed)
    small = rs.randint(0, 256, (n, (H + 7) // 8, (W + 7) // 8, 3)).astype(np.uint8)          # blocky frames: chroma that survives subsampling
    rgb = np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)[:, :H, :W]
    frames = [ref.rgb_to_yuv(x, chroma, "bt601", False) for x in rgb]
    header = ref.y4m_header(W, H, chroma)
    data = ref.y4m_bytes(frames, W, H, chroma, header=header)
    return data, header, frames, [ref.yuv_to_rgb(f, H, W, chroma, "bt601", False) for f in frames]


def _library(route, rgb):
    """what the library route returns for the RGB frames, batch by batch as the driver groups them: a list of (H,W,3) uint8 arrays"""
    net, outs = _net(), []
    B = 2 if route != "tile" else 8
    with torch.no_grad():
        for lo in range(0, len(rgb), B):
            x = torch.from_numpy(np.stack(rgb[lo:lo + B])).to(DEV)
            if route == "plain":
                net.output_u8 = True
                y = net(x)[2]
                net.output_u8 = False
            elif route == "fit":
                y = net.forward_fit(x)[2]
            else:
                y = torch.stack([o[2] for o in net.forward_tiled_many([t for t in x], overlap=16, tile_batch=8, output_u8=True)])
            outs += [a for a in y.cpu().numpy()]
    return outs


def _setup(tmp_path):
    os.makedirs(tmp_path / "ckpt" / NAME, exist_ok=True)
    torch.save(generate_state_dict(evalref.TINY, seed=0), tmp_path / "ckpt" / NAME / "32_net_G.pth")


def _cmd(tmp_path, src, dst, extra):
    return [sys.executable, os.path.join(ROOT, "dehaze_video.py"), "--in", str(src), "--out", str(dst), "--name", NAME, "--n_feats", "24",
            "--hidden_dim_ratio", "4", "--which_epoch", "32", "--loadSize", "64", "--patch_size", "8", "--checkpoints_dir", str(tmp_path / "ckpt")] + extra


def _run(tmp_path, src, dst, extra, **kw):
    return subprocess.run(_cmd(tmp_path, src, dst, extra), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=False, **kw)


def _check_stream(out_bytes, route, header, want_rgb):
    n, H, W, chroma, _ = CASES[route]
    got_header, got = ref.y4m_frames(out_bytes, H, W, chroma)
    assert got_header == header and len(got) == n
    for k in range(n):
        want = ref.rgb_to_yuv(want_rgb[k], chroma, "bt601", False)
        bad = int((got[k] != want).sum())
        print("%s frame %d: %d of %d bytes differ from the library route" % (route, k, bad, want.size))
        assert bad == 0


def _against_test_py(tmp_path, route, rgb, out_bytes):
    from PIL import Image
    n, H, W, chroma, _ = CASES[route]
    data = tmp_path / ("data_" + route)
    os.makedirs(data / "hazy")
    for k, x in enumerate(rgb):
        Image.fromarray(x).save(data / "hazy" / ("frame_%06d.png" % k))
    r = evalref._run_cli(tmp_path, data, NAME, ["--u8_input", "--batchSize", "2"] + (["--fit"] if route == "fit" else []), route)
    assert r.returncode == 0, r.stdout[-3000:]
    _, got = ref.y4m_frames(out_bytes, H, W, chroma)
    for k in range(n):
        png = np.asarray(Image.open(tmp_path / ("res_" + route) / NAME / "test_32" / "images" / ("frame_%06d_fake_A.png" % k)).convert("RGB"))
        assert np.array_equal(ref.rgb_to_yuv(png, chroma, "bt601", False), got[k]), (route, k)


def test_plain_frames_buffers_noref_and_test_py(tmp_path):
    _setup(tmp_path)
    data, header, frames, rgb = _stream("plain")
    (tmp_path / "in.y4m").write_bytes(data)
    r = _run(tmp_path, tmp_path / "in.y4m", tmp_path / "out.y4m", CASES["plain"][4])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    text = r.stdout.decode()
    assert "matrix bt601 (auto" in text and "range limited (auto" in text and "video_matrix: auto" in text
    last = text.strip().splitlines()[-1]
    assert last.startswith("video: 5 frames in ") and last.endswith(" frames/s stream to stream")
    out = (tmp_path / "out.y4m").read_bytes()
    want = _library("plain", rgb)
    _check_stream(out, "plain", header, want)
    # one buffer instead of four, scored on the way: the same bytes, and noref.csv beside the output
    r = _run(tmp_path, tmp_path / "in.y4m", tmp_path / "out1.y4m", CASES["plain"][4] + ["--video_buffers", "1", "--eval_noref"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert (tmp_path / "out1.y4m").read_bytes() == out
    lines = (tmp_path / "noref.csv").read_text().splitlines()
    assert lines[0] == metrics.NOREF_CSV_HEADER and [l.split(",")[0] for l in lines[1:]] == ["frame_%06d" % k for k in range(5)]
    for k, line in enumerate(lines[1:]):
        values = np.array([float(v) for v in line.split(",")[1:]])
        score = noref_ref.scores(rgb[k][None], want[k][None], 7)[0]
        print("frame %d: csv against the restatement, max difference %.3g" % (k, np.abs(values - score).max()))
        assert np.abs(values - score).max() <= 1e-6
    assert not os.path.exists(tmp_path / "out.y4m.csv") and "noref: wrote" in r.stdout.decode()
    _against_test_py(tmp_path, "plain", rgb, out)


def test_fit_frames_and_test_py(tmp_path):
    _setup(tmp_path)
    data, header, frames, rgb = _stream("fit")
    (tmp_path / "in.y4m").write_bytes(data)
    r = _run(tmp_path, tmp_path / "in.y4m", tmp_path / "out.y4m", CASES["fit"][4])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    out = (tmp_path / "out.y4m").read_bytes()
    _check_stream(out, "fit", header, _library("fit", rgb))
    _against_test_py(tmp_path, "fit", rgb, out)


def test_tile_frames(tmp_path):
    _setup(tmp_path)
    data, header, frames, rgb = _stream("tile")
    (tmp_path / "in.y4m").write_bytes(data)
    r = _run(tmp_path, tmp_path / "in.y4m", tmp_path / "out.y4m", CASES["tile"][4])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    _check_stream((tmp_path / "out.y4m").read_bytes(), "tile", header, _library("tile", rgb))


def test_tile_frames_when_the_first_frame_initialises_the_actnorm_layers(tmp_path):
    """a checkpoint as the reference's define_G leaves it: frame 0 runs alone through the model's route (as test.py --tile runs its first image) and
    initialises the layers, the rest of the batch is packed; the test above takes the other branch (a checkpoint with initialised layers)"""
    sd = generate_state_dict(evalref.TINY, seed=0, mode="reference_init")
    assert any(k.endswith("initialized") and int(v) == 0 for k, v in sd.items())
    assert all(int(v) != 0 for k, v in generate_state_dict(evalref.TINY, seed=0).items() if k.endswith("initialized"))
    os.makedirs(tmp_path / "ckpt" / NAME)
    torch.save(sd, tmp_path / "ckpt" / NAME / "32_net_G.pth")
    data, header, frames, rgb = _stream("tile")
    (tmp_path / "in.y4m").write_bytes(data)
    r = _run(tmp_path, tmp_path / "in.y4m", tmp_path / "out.y4m", CASES["tile"][4])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert b"batchSize: 8" in r.stdout and b"batchSize: 1" not in r.stdout                 # what is printed is what runs
    assert os.path.exists(tmp_path / "ckpt" / NAME / "video_opt.txt") and not os.path.exists(tmp_path / "ckpt" / NAME / "opt.txt")
    net = dec_ipt(evalref.TINY, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    x = torch.from_numpy(np.stack(rgb)).to(DEV)
    with torch.no_grad():
        first = net.forward_tiled(x[:1], overlap=16, tile_batch=8, output_u8=True)[2]
        rest = net.forward_tiled_many([x[1]], overlap=16, tile_batch=8, output_u8=True)
    want = [first[0].cpu().numpy(), rest[0][2].cpu().numpy()]
    _check_stream((tmp_path / "out.y4m").read_bytes(), "tile", header, want)


def test_pipes_carry_the_video_alone(tmp_path):
    _setup(tmp_path)
    data, header, frames, rgb = _stream("plain")
    r = _run(tmp_path, "-", "-", CASES["plain"][4], input=data)
    assert r.returncode == 0, r.stderr[-3000:]
    _check_stream(r.stdout, "plain", header, _library("plain", rgb))               # nothing but the stream on stdout
    assert len(r.stdout) == len(data)
    err = r.stderr.decode()
    assert "------------ Options -------------" in err and err.strip().splitlines()[-1].startswith("video: 5 frames in ")


def test_refusals_come_before_any_output(tmp_path):
    _setup(tmp_path)
    data = _stream("fit")[0]
    (tmp_path / "odd.y4m").write_bytes(data)
    frame = bytes(ref.frame_bytes(T, T, "420jpeg"))
    (tmp_path / "deep.y4m").write_bytes(b"YUV4MPEG2 W128 H128 F25:1 Ip A1:1 C420p10\nFRAME\n" + frame + frame)
    (tmp_path / "mixed.y4m").write_bytes(b"YUV4MPEG2 W128 H128 F25:1 Im A1:1 C420jpeg\nFRAME\n" + frame)
    for src, words in (("odd.y4m", ("201 x 150", "128 x 128", "--fit", "--tile")), ("deep.y4m", ("C420p10",)), ("mixed.y4m", ("'Im'", "interlaced"))):
        dst = tmp_path / ("out_" + src)
        r = _run(tmp_path, tmp_path / src, dst, [])
        err = r.stderr.decode()
        assert r.returncode != 0 and all(w in err for w in words), (src, r.returncode, err[-2000:])
        assert not os.path.exists(dst)
        assert "Traceback" not in err
    r = _run(tmp_path, "-", "-", [], input=(tmp_path / "deep.y4m").read_bytes())
    assert r.returncode != 0 and r.stdout == b"" and "C420p10" in r.stderr.decode()
