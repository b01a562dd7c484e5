"""CIEDE2000 (include/cfen_colordiff.h) on the host: the float64 restatement tests/ciede_ref.py against the published test pairs of Sharma, Wu
and Dalal and against anchors of the byte-to-dE chain, the sRGB table the kernel is handed, the header's ledger, the argument errors of the
entry point, the --eval_ciede2000 option and the csv / summary text with the extra column.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import cabi_ledger
import ciede_ref as ref


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def test_sharma_pairs():
    assert ref.SHARMA.shape == (34, 7)
    assert tuple(ref.SHARMA[0]) == (50.0, 2.6772, -79.7751, 50.0, 0.0, -82.7485, 2.0425) and ref.SHARMA[1, 6] == 2.8615 and ref.SHARMA[2, 6] == 3.4412
    got = ref.delta_e_lab(*ref.SHARMA[:, :6].T)
    for row, g in zip(ref.SHARMA, got):
        assert abs(g - row[6]) < 5.1e-5, (row, g)            # the table has four decimals
    swapped = ref.delta_e_lab(*ref.SHARMA[:, [3, 4, 5, 0, 1, 2]].T)
    assert np.abs(swapped - got).max() < 1e-12               # the formula is symmetric


ANCHORS = [((0, 0, 0), (255, 255, 255), 100.000000), ((255, 0, 0), (0, 255, 0), 86.608239), ((255, 0, 0), (0, 0, 255), 52.881365),
           ((127, 127, 127), (128, 128, 128), 0.380552), ((128, 128, 128), (255, 0, 0), 31.196562), ((10, 20, 30), (12, 18, 33), 4.158598)]


@pytest.mark.parametrize("p,q,want", ANCHORS)
def test_byte_anchors(p, q, want):
    got = float(ref.ciede2000_u8(np.array(p, np.uint8), np.array(q, np.uint8)))
    assert abs(got - want) <= 1e-5, got


def test_corner_grid():
    a, b = ref.corner_grid()
    assert a.shape == b.shape == (512, 512, 3) and tuple(a[1, 0]) == (0, 0, 1) == tuple(b[0, 1]) and tuple(a[511, 0]) == (255, 255, 255)
    m = ref.ciede2000_u8(a, b)
    assert not np.isnan(m).any() and abs(m.mean() - 50.254016) <= 1e-5
    assert (np.diag(m) == 0).all() and np.array_equal(m, m.T)
    # the discontinuity: 88 of the 262144 pairs have exactly opposite hues, well under the 1e-3 share a GPU test may exclude
    opp = ref.opposite_hues(a, b)
    assert opp.sum() == 88 and opp.mean() < 1e-3
    bv = ref.branch_values(a, b)
    assert bv.shape == (4, 512, 512) and np.array_equal(bv[0], m) and not np.isnan(bv).any()


def test_white_black_and_greys():
    L, a, b = ref.lab_from_bytes(np.array([[255, 255, 255], [0, 0, 0], [128, 128, 128], [2, 3, 3]], np.uint8))
    assert abs(L[0] - 100.0) <= 1e-9 and L[1] == 0.0
    assert (a[:3] == 0).all() and (b[:3] == 0).all()
    assert abs(np.hypot(a[3], b[3]) - 0.277) < 1e-3          # the smallest chroma of a byte colour that is not grey
    v = np.arange(256, dtype=np.uint8)
    rgb = np.stack(np.meshgrid(v[:8], v[:8], v[:8], indexing="ij"), -1).reshape(-1, 3)
    L, a, b = ref.lab_from_bytes(rgb)
    chroma = np.hypot(a, b)
    grey = (rgb[:, 0] == rgb[:, 1]) & (rgb[:, 1] == rgb[:, 2])
    assert (chroma[grey] == 0).all() and chroma[~grey].min() > 0.27


def test_srgb_linear_table():
    from cfen_vit_dehazing_amd import metrics
    t = metrics.srgb_linear_table()
    assert t.shape == (256,) and t.dtype == np.float32
    assert np.array_equal(t, ref.srgb_linear_table().astype(np.float32))
    c = np.arange(256) / 255.0
    want = [x / 12.92 if x <= 0.04045 else ((x + 0.055) / 1.055) ** 2.4 for x in c.tolist()]
    assert np.array_equal(t, np.array(want, np.float64).astype(np.float32))
    assert t[0] == 0.0 and t[255] == 1.0 and (np.diff(t) > 0).all()
    assert abs(float(t[10]) - 10 / 255.0 / 12.92) < 1e-9 and abs(float(t[11]) - ((11 / 255.0 + 0.055) / 1.055) ** 2.4) < 1e-9     # the two branches meet between 10 and 11


# ---- the header's ledger ---------------------------------------------------------------------------------------------------------------------------
def test_colordiff_header_is_exported_bound_and_apart_from_the_frozen_abi():
    cabi_ledger.check_header_bound("cfen_colordiff.h", {"cfen_ciede2000_bytes": 3, "cfen_ciede2000_u8": 10}, word="ciede")


def test_scratch_size_is_one_double_per_1024_pixels():
    from cfen_vit_dehazing_amd import _lib
    q = _lib.load().cfen_ciede2000_bytes
    for B, H, W in ((1, 1, 1), (2, 3, 5), (3, 17, 67), (1, 32, 32), (1, 32, 33), (2, 97, 131), (8, 512, 512), (1, 2160, 3840), (65535, 65536, 65536)):
        assert q(B, H, W) == B * -(-(H * W) // 1024) * 8, (B, H, W)
    for B, H, W in ((0, 4, 4), (-1, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 0), (1, 65537, 4), (1, 4, 65537)):
        assert q(B, H, W) == 0, (B, H, W)


def test_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    a, b, tab, scr, mp, out, z = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 0))      # never dereferenced
    refused = functools.partial(cabi_ledger.refused, lib, "ciede2000_u8")

    for bad in ((z, b, tab, scr, out), (a, z, tab, scr, out), (a, b, z, scr, out), (a, b, tab, z, out), (a, b, tab, scr, z)):
        refused(b"null pointer", bad[0], bad[1], 1, 4, 4, bad[2], bad[3], mp, bad[4], z)
    refused(b"B = 0", a, b, 0, 4, 4, tab, scr, mp, out, z)
    refused(b"B = -3", a, b, -3, 4, 4, tab, scr, mp, out, z)
    refused(b"B = 65536", a, b, 65536, 4, 4, tab, scr, mp, out, z)
    refused(b"H = 0", a, b, 1, 0, 4, tab, scr, mp, out, z)
    refused(b"W = 0", a, b, 1, 4, 0, tab, scr, mp, out, z)
    refused(b"H = 65537", a, b, 1, 65537, 4, tab, scr, mp, out, z)
    refused(b"W = 65537", a, b, 1, 4, 65537, tab, scr, mp, out, z)
    refused(b"8-byte aligned", a, b, 1, 4, 4, tab, scr, mp, ctypes.c_void_p((6 << 20) + 4), z)
    refused(b"8-byte aligned", a, b, 1, 4, 4, tab, ctypes.c_void_p((4 << 20) + 4), mp, out, z)
    refused(b"4-byte aligned", a, b, 1, 4, 4, ctypes.c_void_p((3 << 20) + 2), scr, mp, out, z)
    refused(b"4-byte aligned", a, b, 1, 4, 4, tab, scr, ctypes.c_void_p((5 << 20) + 1), out, z)


# ---- options -----------------------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ckpt"), "--gpu_ids", "-1"] + extra)


def test_eval_ciede2000_needs_eval_and_stays_out_of_the_way(tmp_path, capsys):
    with pytest.raises(ValueError, match="--eval_ciede2000.*needs --eval"):
        _parse(tmp_path, ["--sb", "--eval_ciede2000"])
    capsys.readouterr()
    opt = _parse(tmp_path, ["--sb", "--eval", "--eval_ciede2000"])
    assert opt.eval_ciede2000 is True and opt.eval_metrics == "psnr,ssim"
    keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
    assert "eval_ciede2000" in keys and "eval_metrics" not in keys
    opt = _parse(tmp_path, ["--sb", "--eval", "--eval_ciede2000", "--eval_metrics", "psnr,ssim,msssim", "--tile", "--self_ensemble", "--gpu_png"])
    assert opt.eval_ciede2000 is True and opt.eval_metrics == "psnr,ssim,msssim"
    capsys.readouterr()
    for extra in (["--sb", "--eval"], ["--sb"]):
        opt = _parse(tmp_path, extra)
        assert opt.eval_ciede2000 is False
        keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
        assert "eval_ciede2000" not in keys and "tile" in keys          # a run without the flag prints the options it always printed
        assert "eval_ciede2000" not in [line.split(":")[0] for line in open(tmp_path / "ckpt" / opt.name / "opt.txt").read().splitlines()]
    with pytest.raises(ValueError, match="ciede2000") as e:              # still not a name of --eval_metrics; the message now says where it went
        _parse(tmp_path, ["--sb", "--eval", "--eval_metrics", "psnr,ssim,ciede2000"])
    assert "unknown metric 'ciede2000'" in str(e.value) and "--eval_ciede2000" in str(e.value)
    with pytest.raises(ValueError) as e:
        _parse(tmp_path, ["--sb", "--eval", "--eval_metrics", "psnr,ssim,lpips"])
    assert "--eval_ciede2000" not in str(e.value)
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    o = TestOptions()
    o.initialize()
    action = next(a for a in o.parser._actions if "--eval_ciede2000" in a.option_strings)
    assert action.help.startswith("(extension)") and action.default is False


# ---- csv -----------------------------------------------------------------------------------------------------------------------------------------------
def test_csv_text_and_summary_with_the_ciede_column():
    from cfen_vit_dehazing_amd import metrics
    assert metrics.COLUMNS == ("psnr", "ssim", "msssim") and metrics.CIEDE_COLUMN == "ciede2000" and metrics.CSV_HEADER == "image,psnr,ssim"
    rows2 = [("1400_1.png", 23.4567891, 0.9123456789), ("same.png", float("inf"), 1.0), ("b.png", 10.0, 0.5)]
    rows3m = [("1400_1.png", 23.4567891, 0.9123456789, 0.95), ("same.png", float("inf"), 1.0, 1.0), ("b.png", 10.0, 0.5, float("nan"))]
    two, three = ("psnr", "ssim"), ("psnr", "ssim", "msssim")
    # the old outputs, byte for byte
    assert metrics.format_csv_columns(rows2, two) == metrics.format_csv(rows2) == \
        "image,psnr,ssim\n1400_1.png,23.456789,0.912346\nsame.png,inf,1.000000\nb.png,10.000000,0.500000\n"
    assert metrics.format_csv_columns(rows3m, three) == \
        "image,psnr,ssim,msssim\n1400_1.png,23.456789,0.912346,0.950000\nsame.png,inf,1.000000,1.000000\nb.png,10.000000,0.500000,nan\n"
    assert metrics.summary_line_columns(rows2, two) == metrics.summary_line(rows2) == \
        "eval: 3 images, mean PSNR 16.7284 dB over 2 finite (1 infinite), mean SSIM 0.804115"
    assert metrics.summary_line_columns(rows3m, three) == metrics.summary_line(rows2) + ", mean MS-SSIM 0.975000 over 2 (1 nan)"
    assert metrics.summarize_columns(rows2, two) == metrics.summarize(rows2) and "ciede2000_mean" not in metrics.summarize_columns(rows3m, three)
    # three columns: psnr, ssim, ciede2000
    de = (4.1585984, 0.0, 31.25)
    rows3 = [r + (d,) for r, d in zip(rows2, de)]
    cols3 = two + ("ciede2000",)
    assert metrics.format_csv_columns(rows3, cols3) == \
        "image,psnr,ssim,ciede2000\n1400_1.png,23.456789,0.912346,4.158598\nsame.png,inf,1.000000,0.000000\nb.png,10.000000,0.500000,31.250000\n"
    s = metrics.summarize_columns(rows3, cols3)
    assert abs(s["ciede2000_mean"] - sum(de) / 3) < 1e-12 and "msssim_mean" not in s
    assert {k: v for k, v in s.items() if k != "ciede2000_mean"} == metrics.summarize(rows2)
    assert metrics.summary_line_columns(rows3, cols3) == metrics.summary_line(rows2) + ", mean CIEDE2000 11.8029"
    # four columns: psnr, ssim, msssim, ciede2000
    rows4 = [r + (d,) for r, d in zip(rows3m, de)]
    cols4 = three + ("ciede2000",)
    assert metrics.format_csv_columns(rows4, cols4) == ("image,psnr,ssim,msssim,ciede2000\n1400_1.png,23.456789,0.912346,0.950000,4.158598\n"
                                                        "same.png,inf,1.000000,1.000000,0.000000\nb.png,10.000000,0.500000,nan,31.250000\n")
    s = metrics.summarize_columns(rows4, cols4)
    assert abs(s["ciede2000_mean"] - sum(de) / 3) < 1e-12 and s["msssim_nan"] == 1
    assert metrics.summary_line_columns(rows4, cols4) == metrics.summary_line_columns(rows3m, three) + ", mean CIEDE2000 11.8029"
    assert metrics.format_csv_columns([], cols4) == "image,psnr,ssim,msssim,ciede2000\n"
    assert np.isnan(metrics.summarize_columns([], cols3)["ciede2000_mean"])
    with pytest.raises(ValueError):
        metrics.format_csv_columns(rows3m, cols4)


def test_ciede2000_needs_cuda_tensors():
    import torch
    from cfen_vit_dehazing_amd import metrics
    z = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="ciede2000 needs CUDA tensors; there is no CPU fallback"):
        metrics.ciede2000(z, z)
    with pytest.raises(ValueError, match="ciede2000 needs CUDA tensors"):
        metrics.ciede2000(z.numpy(), z.numpy())
