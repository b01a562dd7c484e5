"""CIEDE2000 on the device (cfen_ciede2000_u8; ops.image_ciede2000, metrics.ciede2000, test.py --eval --eval_ciede2000) against the float64
restatement tests/ciede_ref.py, and the second half of the ledger of include/cfen_colordiff.h.

Tolerances (fixed before the kernel ran; a float32 numpy restatement of the header's formula, never the kernel, was measured against float64):
  per pixel  |map - ref| <= 1e-3: the restatement's worst error was 2.9e-4 on a million random pairs and 3.8e-4 on the corner grid outside its
             excluded pairs; 1e-3 leaves about 2.6 x for a device math library that is not numpy's.
  per image  |out - mean(ref)| <= 1e-4: the restatement's mean error was <= 3e-6, and one dropped or doubled pixel moves the mean of the 64 x 64
             case by >= 2.7e-4.
  excluded   CIEDE2000 is discontinuous where the two hues are exactly opposite.  A pixel may skip the per-pixel check only if both colours are
             chromatic and ||h1' - h2'| - 180| < 0.01 degrees in float64; it must then lie within 1e-3 of one of the four branch values
             (ciede_ref.branch_values), and no image may have more than 1e-3 of its pixels excluded."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, metrics, ops
from cfen_vit_dehazing_amd.manifest import generate_state_dict
import cabi_ledger
import ciede_ref as ref
import guarded
import test_hip_metrics as evalref                     # TINY, _run_cli, _dataset: the fixtures of the --eval CLI tests

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL_PIXEL, TOL_IMAGE, MAX_EXCLUDED = 1e-3, 1e-4, 1e-3


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared reference arrays are read-only


def _random(shape, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, shape + (3,), dtype=np.uint8), rs.randint(0, 256, shape + (3,), dtype=np.uint8)


def _near(shape, seed):
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, shape + (3,), dtype=np.uint8)
    return a, np.clip(a.astype(np.int64) + rs.randint(-6, 7, a.shape), 0, 255).astype(np.uint8)


def _grey_colour(shape, seed):
    rs = np.random.RandomState(seed)
    return np.repeat(rs.randint(0, 256, shape + (1,), dtype=np.uint8), 3, axis=-1), rs.randint(0, 256, shape + (3,), dtype=np.uint8)


def _corner(shape, seed):
    a, b = ref.corner_grid()
    return a[None], b[None]


# (B, H, W): 1024 pixels per workgroup, 4 per thread
CASES = {
    "1x1x1": (_random, (1, 1, 1)),                     # the smallest input
    "2x3x5": (_random, (2, 3, 5)),                     # a small batch with a tail
    "3x17x67": (_random, (3, 17, 67)),                 # image stride 3417 bytes: images 1 and 2 start misaligned -- byte path and tails
    "1x64x64": (_random, (1, 64, 64)),                 # all on the vector path
    "2x97x131": (_random, (2, 97, 131)),               # 12707 pixels: a tail in every image's last workgroup, odd map offsets
    "corner_grid": (_corner, (1, 512, 512)),           # 256 partials: every finish thread has exactly one
    "1x520x517": (_random, (1, 520, 517)),             # 263 partials: more than the finish workgroup has threads
    "near_64": (_near, (1, 64, 64)),                   # +-6 levels
    "grey_colour_64": (_grey_colour, (1, 64, 64)),     # a grey against a colour
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(a, b, ref64 (B,H,W), excluded mask, branch values (4,B,H,W)): computed once, shared, read-only"""
    gen, shape = CASES[name]
    a, b = gen(shape, sum(shape) + len(name))
    assert a.shape == shape + (3,) == b.shape
    out = (a, b, ref.ciede2000_u8(a, b), ref.opposite_hues(a, b), ref.branch_values(a, b))
    for x in out:
        x.setflags(write=False)
    return out


def check(name, out, dmap):
    a, b, want, opp, branches = case(name)
    B = a.shape[0]
    got = dmap.cpu().numpy().astype(np.float64)
    means = out.cpu().numpy()
    assert got.shape == want.shape and means.shape == (B,) and dmap.dtype == torch.float32 and out.dtype == torch.float64
    assert not np.isnan(got).any() and not np.isnan(means).any()
    err = np.abs(got - want)
    branch_err = np.abs(got[None] - branches).min(axis=0)
    excluded = [float(opp[i].mean()) for i in range(B)]
    image_err = [abs(means[i] - want[i].mean()) for i in range(B)]
    print("%s: per pixel max |map - ref| %.3e outside %d excluded pixels (at most %.2e of an image), excluded pixels within %.3e of a branch; "
          "per image max |out - mean(ref)| %.3e" % (name, err[~opp].max() if (~opp).any() else 0.0, opp.sum(), max(excluded),
                                                    branch_err[opp].max() if opp.any() else 0.0, max(image_err)))
    assert max(excluded) <= MAX_EXCLUDED
    assert (err[~opp] <= TOL_PIXEL).all()
    assert (branch_err[opp] <= TOL_PIXEL).all()
    assert max(image_err) <= TOL_IMAGE
    # the mean is the fp64 sum of the fp32 map values over H W
    mean_of_map = dmap.double().flatten(1).mean(dim=1).cpu().numpy()
    assert (np.abs(means - mean_of_map) <= 1e-12 * np.abs(mean_of_map)).all()


# ---- against float64 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(name):
    a, b = case(name)[:2]
    ta, tb = dev(a), dev(b)
    out, dmap = ops.image_ciede2000(ta, tb, map=True)
    check(name, out, dmap)
    # without a map, and with a caller-placed one: the same bits
    alone = ops.image_ciede2000(ta, tb)
    placed = torch.full(a.shape[:3], float("nan"), dtype=torch.float32, device=DEV)
    out2, map2 = ops.image_ciede2000(ta, tb, map=placed, out=torch.empty(a.shape[0], dtype=torch.float64, device=DEV))
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, out) and torch.equal(out2, out)
    assert map2.data_ptr() == placed.data_ptr() and torch.equal(map2, dmap)


def test_paths_the_cases_claim():
    assert (17 * 67 * 3) % 4 == 1 and (97 * 131 * 3) % 4 == 1 and (64 * 64) % 1024 == 0          # misaligned second images; whole workgroups
    assert (97 * 131) % 4 == 3 and (97 * 131 * 4) % 16 == 12                                    # a 3-pixel tail; image 1's map is not 16-byte aligned
    q = _lib.load().cfen_ciede2000_bytes
    assert q(1, 512, 512) == 256 * 8 and q(1, 520, 517) == 263 * 8 and q(1, 1, 1) == 8


@pytest.mark.parametrize("name", ["3x17x67", "1x64x64", "corner_grid"])
def test_equal_images_score_exactly_zero(name):
    for img in case(name)[:2]:
        t = dev(img)
        out, dmap = ops.image_ciede2000(t, t.clone(), map=True)
        assert not bool(dmap.view(torch.int32).any()) and not bool(out.view(torch.int64).any())          # +0.0 bitwise, so no NaN either


def test_batch_stream_and_alignment_do_not_change_a_bit():
    a, b = case("3x17x67")[:2]
    ta, tb = dev(a), dev(b)
    out, dmap = ops.image_ciede2000(ta, tb, map=True)
    one = [ops.image_ciede2000(ta[i:i + 1].clone(), tb[i:i + 1].clone(), map=True) for i in range(3)]          # (each clone is aligned: the vector path)
    assert torch.equal(out, torch.cat([o[0] for o in one])) and torch.equal(dmap, torch.cat([o[1] for o in one]))
    again = ops.image_ciede2000(ta, tb, map=True)
    assert torch.equal(out, again[0]) and torch.equal(dmap, again[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.image_ciede2000(ta, tb, map=True)
    side.synchronize()
    assert torch.equal(out, other[0]) and torch.equal(dmap, other[1])
    # views at a 1-byte offset into a larger buffer
    n = ta.numel()
    ba, bb = torch.zeros(n + 1, dtype=torch.uint8, device=DEV), torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    ba[1:].copy_(ta.flatten())
    bb[1:].copy_(tb.flatten())
    va, vb = ba[1:].view(ta.shape), bb[1:].view(tb.shape)
    assert va.data_ptr() % 4 == 1 and va.is_contiguous()
    off = ops.image_ciede2000(va, vb, map=True)
    assert torch.equal(out, off[0]) and torch.equal(dmap, off[1])
    mixed = ops.image_ciede2000(va, tb, map=True)                    # the choice is made per input
    assert torch.equal(out, mixed[0]) and torch.equal(dmap, mixed[1])
    check("3x17x67", out, dmap)


# ---- guard bands and the header's ledger -----------------------------------------------------------------------------------------------------------
def test_guard_bands_ciede():
    """both inputs and the table between 0xff bands; scratch, map and out prefilled 0xff (NaN) between random bands: no band changes, the results
    are the unguarded call's, a zero prefill gives the same, and without a map nothing but scratch and out is written"""
    lib = _lib.load()
    table = guarded.guarded_copy(dev(metrics.srgb_linear_table()))
    for name in ("3x17x67", "2x97x131"):                                   # byte path and tails; vector path with 13 workgroups per image
        a, b = case(name)[:2]
        B, H, W = a.shape[:3]
        ta, tb = guarded.guarded_copy(dev(a)), guarded.guarded_copy(dev(b))
        nbytes = lib.cfen_ciede2000_bytes(B, H, W)
        assert nbytes == B * -(-(H * W) // 1024) * 8
        scratch = guarded.guarded_empty((nbytes // 8,), torch.float64, DEV, fill="ff")
        dmap = guarded.guarded_empty((B, H, W), torch.float32, DEV, fill="ff")
        out = guarded.guarded_empty((B,), torch.float64, DEV, fill="ff")
        want, want_map = ops.image_ciede2000(dev(a), dev(b), map=True)
        for fill in ("ff", "zero"):
            for t in (scratch, dmap, out):
                guarded.refill(t, fill)
            _lib.check(lib.cfen_ciede2000_u8(_lib.ptr(ta), _lib.ptr(tb), B, H, W, _lib.ptr(table), _lib.ptr(scratch), _lib.ptr(dmap), _lib.ptr(out),
                                             _lib.current_stream()), "ciede2000_u8")
            torch.cuda.synchronize()
            guarded.check_bands(ta, tb, table, scratch, dmap, out)
            assert bool(torch.isfinite(scratch).all()) and torch.equal(out, want) and torch.equal(dmap, want_map), (name, fill)
        for t in (scratch, dmap, out):
            guarded.refill(t, "ff")
        _lib.check(lib.cfen_ciede2000_u8(_lib.ptr(ta), _lib.ptr(tb), B, H, W, _lib.ptr(table), _lib.ptr(scratch), None, _lib.ptr(out),
                                         _lib.current_stream()), "ciede2000_u8")
        torch.cuda.synchronize()
        guarded.check_bands(ta, tb, table, scratch, dmap, out)
        assert torch.equal(out, want) and bool((guarded.raw_bytes(dmap) == 255).all())
        check(name, out, want_map)


def test_every_function_of_the_colordiff_header_is_guard_band_tested():
    fns = cabi_ledger.header_functions("cfen_colordiff.h")
    assert sorted(fns) == sorted(_lib.HEADERS["cfen_colordiff.h"])
    cabi_ledger.check_guard_band_test_calls("test_hip_ciede.py", "test_guard_bands_ciede", fns)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    lib = _lib.load()
    B, H, W = 2, 3, 5
    a, b = (dev(x) for x in case("2x3x5")[:2])
    table = dev(metrics.srgb_linear_table())
    scratch = torch.full((B,), 7.0, dtype=torch.float64, device=DEV)
    dmap = torch.full((B, H, W), 7.0, dtype=torch.float32, device=DEV)
    out = torch.full((B + 1,), 7.0, dtype=torch.float64, device=DEV)
    p, z = _lib.ptr, ctypes.c_void_p(0)
    good = dict(a=p(a), b=p(b), B=B, H=H, W=W, table=p(table), scratch=p(scratch), map=p(dmap), out=p(out))
    bad = [(k, z, b"null pointer") for k in ("a", "b", "table", "scratch", "out")]
    bad += [("B", 0, b"B = 0"), ("B", -1, b"B = -1"), ("B", 65536, b"B = 65536"), ("H", 0, b"H = 0"), ("W", 0, b"W = 0"), ("H", 65537, b"H = 65537"),
            ("W", 65537, b"W = 65537"), ("H", -4, b"H = -4"),
            ("out", ctypes.c_void_p(out.data_ptr() + 4), b"8-byte aligned"), ("scratch", ctypes.c_void_p(scratch.data_ptr() + 4), b"8-byte aligned"),
            ("map", ctypes.c_void_p(dmap.data_ptr() + 2), b"4-byte aligned"), ("table", ctypes.c_void_p(table.data_ptr() + 1), b"4-byte aligned")]
    for key, value, what in bad:
        args = dict(good, **{key: value})
        rc = lib.cfen_ciede2000_u8(args["a"], args["b"], args["B"], args["H"], args["W"], args["table"], args["scratch"], args["map"], args["out"],
                                   _lib.current_stream())
        err = lib.cfen_last_error()
        assert rc == -1 and b"ciede2000_u8" in err and what in err, (key, rc, err)
    torch.cuda.synchronize()
    assert bool((scratch == 7.0).all()) and bool((dmap == 7.0).all()) and bool((out == 7.0).all())
    _lib.check(lib.cfen_ciede2000_u8(*[good[k] for k in ("a", "b", "B", "H", "W", "table", "scratch", "map", "out")], _lib.current_stream()), "ciede2000_u8")
    torch.cuda.synchronize()
    assert bool((out[:B] != 7.0).all()) and float(out[B]) == 7.0 and bool((dmap != 7.0).all())


def test_python_side_refusals():
    u = torch.zeros(1, 4, 6, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="differ"):
        ops.image_ciede2000(u, torch.zeros(1, 4, 7, 3, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="uint8"):
        ops.image_ciede2000(u.float(), u.float())
    with pytest.raises(ValueError, match=r"\(B,H,W,3\)"):
        ops.image_ciede2000(u[..., :2].contiguous(), u[..., :2].contiguous())
    with pytest.raises(ValueError, match="contiguous"):
        ops.image_ciede2000(u.cpu(), u.cpu())
    with pytest.raises(ValueError, match="map"):
        ops.image_ciede2000(u, u, map=torch.zeros(1, 4, 6, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        ops.image_ciede2000(u, u, out=torch.zeros(2, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="CUDA tensors"):
        metrics.ciede2000(u.cpu(), u.cpu())
    assert ops.image_ciede2000(u[0], u[0]).tolist() == [0.0]                                    # an image without the batch dimension
    a, b, want = case("2x3x5")[:3]
    got = metrics.ciede2000(dev(a), dev(b))
    assert isinstance(got, list) and all(isinstance(v, float) for v in got) and np.abs(np.array(got) - want.mean(axis=(1, 2))).max() <= TOL_IMAGE


# ---- CLI ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_eval_ciede2000_adds_the_last_column_and_changes_nothing_else(tmp_path):
    from PIL import Image
    name = "iid_hlgvit_crs_gd4_cfs_v3_eval"
    os.makedirs(tmp_path / "ckpt" / name)
    torch.save(generate_state_dict(evalref.TINY, seed=0), tmp_path / "ckpt" / name / "32_net_G.pth")
    data = tmp_path / "data"
    pairs = evalref._dataset(data, (128, 128), seed=5)
    extra = ["--batchSize", "2", "--eval"]
    r = evalref._run_cli(tmp_path, data, name, extra + ["--eval_ciede2000"], "de")
    assert r.returncode == 0, r.stdout[-3000:]
    assert "eval_ciede2000: True" in r.stdout
    res = tmp_path / "res_de" / name / "test_32"
    lines = open(res / "metrics.csv").read().splitlines()
    assert lines[0] == "image,psnr,ssim,ciede2000" and [l.split(",")[0] for l in lines[1:]] == sorted(pairs)
    values = []
    for line in lines[1:]:
        image, _, _, de = line.split(",")
        out = np.asarray(Image.open(res / "images" / (os.path.splitext(image)[0] + "_fake_A.png")).convert("RGB"))
        gt = np.asarray(Image.open(data / "clear" / pairs[image]).convert("RGB"))
        want = float(ref.ciede2000_u8(out, gt).mean())
        print("%s: csv ciede2000 %s, float64 from the files: %.9f" % (image, de, want))
        assert abs(float(de) - want) <= TOL_IMAGE
        values.append(float(de))
    summary = [l for l in r.stdout.splitlines() if l.startswith("eval: ") and "mean PSNR" in l]
    assert len(summary) == 1 and summary[0].endswith(", mean CIEDE2000 %.4f" % (sum(values) / len(values)))
    # the same command without the flag: the same PNG bytes, the csv it always wrote, equal to the first columns, the option list it always printed
    r2 = evalref._run_cli(tmp_path, data, name, extra, "plain")
    assert r2.returncode == 0, r2.stdout[-3000:]
    assert "CIEDE2000" not in r2.stdout and "eval_ciede2000" not in [l.split(":")[0] for l in r2.stdout.splitlines()]
    plain = tmp_path / "res_plain" / name / "test_32"
    old = open(plain / "metrics.csv").read().splitlines()
    assert old[0] == "image,psnr,ssim" and old == [l.rsplit(",", 1)[0] for l in lines]
    assert summary[0].startswith([l for l in r2.stdout.splitlines() if l.startswith("eval: ") and "mean PSNR" in l][0])
    files = sorted(os.listdir(res / "images"))
    assert files == sorted(os.listdir(plain / "images")) and len(files) == 3
    for f in files:
        assert open(res / "images" / f, "rb").read() == open(plain / "images" / f, "rb").read(), f
