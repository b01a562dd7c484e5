"""Guided upsampling (include/cfen_guided.h) on the host: the numpy restatement tests/guided_ref.py against its own brute-force form and against
torch's bilinear interpolation, the properties of the definition, the synthetic scattering-model experiment of DESIGN section 14, the tolerance
TAU of tests/test_hip_guided.py, the argument errors of the two entry points, the --fit_refine options, and the header's ledger.  No GPU."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import cabi_ledger
import guided_ref as ref
import resample_ref

# The tolerance of tests/test_hip_guided.py, in levels (1 = one step of a byte): 8 x the largest |v_float32 - v_float64| of the pre-rounding value v
# over every case of that file, where float32 is the header's formulas rounded to fp32 step by step on the CPU (guided_ref, dtype=float32) --
# never the kernels.  The factor 8 is for the kernels' different summation order in the fp32 box mean (up to 1089 terms) and fused multiply-adds.
# A coefficient case has no full-resolution guide: its v is abar * I + bbar, the model at the low-resolution guide itself.
# Measured: 1.614e-4 (the case 12x14_20x31_binary, whose |Abar| reaches 4; 4.9e-5 over all the others).  test_tau recomputes it.
TAU = 1.29e-3


# ---- the restatement against itself --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,r", [(1, 1, 1), (5, 7, 16), (9, 4, 2)])
def test_cumulative_sums_equal_brute_force(h, w, r):
    I, P = (x[0] for x in ref.lowres("random", 1, h, w, h * w + r))
    fast, brute = ref.statistics(I, P, r), ref.statistics(I, P, r, ref.box_sum_brute)
    for f, b in zip(fast, brute):
        assert f.dtype == np.int64 and np.array_equal(f, b)
    N = fast[0]
    assert N.min() >= 1 and N.max() <= (2 * r + 1) ** 2 and N[0, 0] == min(r + 1, h) * min(r + 1, w)
    for eps in ref.EPS:
        for f, b in zip(ref.smoothed(I, P, r, eps), ref.smoothed(I, P, r, eps, brute=True)):
            assert np.abs(f - b).max() <= 1e-12
        for f, b in zip(ref.smoothed(I, P, r, eps, np.float32), ref.smoothed(I, P, r, eps)):      # the fp32 form is the same function
            assert f.dtype == np.float32 and np.abs(f * 255.0 - b * 255.0).max() <= 1e-2


@pytest.mark.parametrize("src,dst", [((5, 7), (37, 53)), ((33, 40), (16, 16)), ((33, 40), (33, 97)), ((1, 1), (3, 5))])
def test_upsampling_equals_torch_bilinear(src, dst):
    # torch computes the source coordinate in float64, scale * (i + 0.5) - 0.5, good to about 1e-14 of a source pixel at these sizes; neighbours
    # that differ by up to 100 keep that, and the rounding of the lerp itself, under the 1e-12 of the comparison
    c = np.random.RandomState(sum(src + dst)).uniform(-50, 50, src + (6,))
    want = torch.nn.functional.interpolate(torch.from_numpy(c).permute(2, 0, 1)[None], size=dst, mode="bilinear", align_corners=False)
    got = ref.upsample(c, dst[0], dst[1])
    assert got.shape == dst + (6,) and np.abs(got - want[0].permute(1, 2, 0).numpy()).max() <= 1e-12


def test_coordinates_are_exact_integers():
    """at 2160 from 512 the coordinate of row 2000 is 473 + 2992 / 4320; fy comes from one division of two exact integers"""
    y0, y1, fy = ref.axis_coords(512, 2160)
    assert y0[2000] == 473 and y1[2000] == 474 and fy[2000] == (4001 * 512 - 2160 - 473 * 4320) / 4320.0
    assert y0[0] == 0 and fy[0] == 0 and y0[-1] == 511 and y1[-1] == 511
    f32 = ref.axis_coords(512, 2160, np.float32)[2]
    assert f32.dtype == np.float32 and f32[2000] == np.float32(2992) / np.float32(4320)


@pytest.mark.parametrize("c", [0, 1, 128, 255])
def test_constant_output_stays_constant(c):
    G = ref.hires("random", 1, 23, 31, c)[0]
    I = ref.lowres("random", 1, 9, 11, c)[0][0]
    P = np.full((9, 11, 3), c, np.uint8)
    for dtype in (np.float64, np.float32):
        for r, eps in ((1, 1e-4), (2, 1e-4), (16, 1e-2)):
            a, b = ref.coefficients(I, P, r, eps, dtype)
            assert not a.any() and (b == c).all()
            assert (ref.guided_upsample(G, I, P, r, eps, dtype) == c).all()


def test_constant_guide_gives_zero_slope():
    P = ref.lowres("random", 1, 9, 11, 3)[1][0]
    for g in (0, 7, 255):
        for dtype in (np.float64, np.float32):
            a, b = ref.coefficients(np.full((9, 11, 3), g, np.uint8), P, 2, 1e-4, dtype)
            assert not a.any() and np.isfinite(b).all()


# ---- the experiment behind the defaults -----------------------------------------------------------------------------------------------------------
SCENES = {(192, 288, 64, 1): (26.62, 43.85, 41.37, 30.80), (160, 224, 48, 2): (26.50, 42.48, 38.90, 30.72)}


@pytest.mark.parametrize("scene", list(SCENES))
def test_scattering_model_scene(scene):
    """a synthetic scene I = J t + A (1 - t); the hazy image and its ideal dehazed image both go to T x T with PIL's bicubic
    filter; the dehazed one comes back by PIL's bicubic filter, or by guided upsampling against the full-resolution hazy image.  PSNR against the
    ideal: at the defaults guided upsampling is at least 10 dB above bicubic (it is about 17 dB above); the four figures DESIGN quotes are pinned
    to 0.01 dB: bicubic, guided at (r 2, eps 1e-4), (r 4, eps 1e-4), (r 2, eps 1e-3)"""
    H, W, T, seed = scene
    J, I = ref.scattering_scene(H, W, seed)
    J8, G = ref.to_bytes(J), ref.to_bytes(I)
    Ilo, Plo = resample_ref.pil_resize(G, (T, T)), resample_ref.pil_resize(J8, (T, T))
    bicubic = ref.psnr(resample_ref.pil_resize(Plo, (H, W)), J8)
    guided = [ref.psnr(ref.guided_upsample(G, Ilo, Plo, r, eps), J8) for r, eps in ((2, 1e-4), (4, 1e-4), (2, 1e-3))]
    print("scene %s: bicubic %.2f dB, guided %s" % (scene, bicubic, ["%.2f" % g for g in guided]))
    assert guided[0] >= bicubic + 10
    assert np.allclose([bicubic] + guided, SCENES[scene], atol=0.01)


# ---- the tolerance ---------------------------------------------------------------------------------------------------------------------------------
def test_tau():
    worst = {}
    for name, (B, h, w, r) in ref.COEF_CASES.items():
        for kind in ref.KINDS:
            for eps in ref.EPS:
                I, P, a64, b64 = ref.coef_case(name, kind, eps)
                for i in range(B):
                    a32, b32 = ref.smoothed(I[i], P[i], r, eps, np.float32)
                    d = np.abs((a32 * I[i].astype(np.float32) + b32).astype(np.float64) - (a64[i] * I[i] + b64[i])).max()
                    worst["coef " + name] = max(worst.get("coef " + name, 0.0), float(d))
    for name, (_, _, r, _) in ref.APPLY_CASES.items():
        G, I, P, v64 = ref.apply_case(name)
        v32 = ref.guided_v(G[0], I[0], P[0], r, 1e-4, np.float32)
        worst["apply " + name] = float(np.abs(v32.astype(np.float64) - v64[0]).max())
    top = max(worst.values())
    print("max |v32 - v64| = %.4e (%s); TAU = %.3e = %.2f x" % (top, max(worst, key=worst.get), TAU, TAU / top))
    assert 4 * top <= TAU <= 16 * top


# ---- the C entry points refuse bad arguments before any launch --------------------------------------------------------------------------------------
def test_guided_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    g, s, tmp, coef, hi, dst, z = (ctypes.c_void_p(v) for v in (1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20, 0))      # never dereferenced
    f = ctypes.c_float
    refused = functools.partial(cabi_ledger.refused, lib)

    ok = 6.5
    for bad in ((z, s, tmp, coef), (g, z, tmp, coef), (g, s, z, coef), (g, s, tmp, z)):
        refused("guided_coef_u8", b"null pointer", bad[0], bad[1], 1, 4, 4, 2, f(ok), bad[2], bad[3], z)
    refused("guided_coef_u8", b"B = 0", g, s, 0, 4, 4, 2, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"B = 65537", g, s, 65537, 4, 4, 2, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"radius = 0", g, s, 1, 4, 4, 0, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"radius = 17", g, s, 1, 4, 4, 17, f(ok), tmp, coef, z)
    for eps in (0.0, -1.0, math.nan, math.inf):
        refused("guided_coef_u8", b"eps255", g, s, 1, 4, 4, 2, f(eps), tmp, coef, z)
    refused("guided_coef_u8", b"h = 0", g, s, 1, 0, 4, 2, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"w = 16385", g, s, 1, 4, 16385, 2, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"must not overlap", g, s, 1, 4, 4, 2, f(ok), tmp, tmp, z)
    refused("guided_coef_u8", b"must not overlap", g, s, 1, 4, 4, 2, f(ok), tmp, ctypes.c_void_p((3 << 20) + 16), z)      # partly overlapping
    refused("guided_coef_u8", b"must not overlap", g, g, 1, 4, 4, 2, f(ok), tmp, coef, z)
    refused("guided_coef_u8", b"16-byte aligned", g, s, 1, 4, 4, 2, f(ok), ctypes.c_void_p((3 << 20) + 4), coef, z)

    for bad in ((z, hi, dst), (coef, z, dst), (coef, hi, z)):
        refused("guided_apply_u8", b"null pointer", bad[0], 1, 4, 4, bad[1], 8, 8, bad[2], z)
    refused("guided_apply_u8", b"B = 0", coef, 0, 4, 4, hi, 8, 8, dst, z)
    refused("guided_apply_u8", b"w = 0", coef, 1, 4, 0, hi, 8, 8, dst, z)
    refused("guided_apply_u8", b"H = 0", coef, 1, 4, 4, hi, 0, 8, dst, z)
    refused("guided_apply_u8", b"W = 16385", coef, 1, 4, 4, hi, 8, 16385, dst, z)
    refused("guided_apply_u8", b"h = 16385", coef, 1, 16385, 4, hi, 8, 8, dst, z)
    refused("guided_apply_u8", b"must not overlap", coef, 1, 4, 4, hi, 8, 8, hi, z)
    refused("guided_apply_u8", b"must not overlap", coef, 1, 4, 4, hi, 8, 8, ctypes.c_void_p((5 << 20) + 191), z)       # dst begins in guide_hi's last byte
    refused("guided_apply_u8", b"must not overlap", coef, 1, 4, 4, hi, 8, 8, coef, z)
    refused("guided_apply_u8", b"16-byte aligned", ctypes.c_void_p((4 << 20) + 8), 1, 4, 4, hi, 8, 8, dst, z)


# ---- --fit_refine at option parsing ------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--name", "fit", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_fit_refine_flags_and_refusals(tmp_path, capsys):
    opt = _parse(tmp_path)
    assert opt.fit_refine == "none" and opt.fit_radius == 2 and opt.fit_eps == 1e-4
    assert "fit_refine:" not in capsys.readouterr().out              # a run without the flag prints what it always did
    opt = _parse(tmp_path, "--fit")
    assert opt.fit_refine == "none"
    opt = _parse(tmp_path, "--fit", "--fit_refine", "guided", "--fit_radius", "16", "--fit_eps", "0.01", "--batchSize", "4", "--u8_input", "--eval", "--sb")
    assert opt.fit_refine == "guided" and opt.fit_radius == 16 and opt.fit_eps == 0.01
    assert "fit_refine: guided" in capsys.readouterr().out
    for extra, names in ((["--fit_refine", "guided"], ("--fit_refine", "--fit")),
                         (["--fit", "--fit_refine", "guided", "--fit_radius", "0"], ("--fit_radius",)),
                         (["--fit", "--fit_refine", "guided", "--fit_radius", "17"], ("--fit_radius",)),
                         (["--fit", "--fit_refine", "guided", "--fit_eps", "0"], ("--fit_eps",)),
                         (["--fit", "--fit_refine", "guided", "--fit_eps=-1e-4"], ("--fit_eps",)),
                         (["--fit", "--fit_refine", "guided", "--fit_eps", "nan"], ("--fit_eps",)),
                         (["--fit", "--fit_refine", "guided", "--fit_eps", "inf"], ("--fit_eps",)),
                         (["--fit", "--fit_refine", "guided", "--tile"], ("--fit", "--tile"))):
        with pytest.raises(ValueError) as e:
            _parse(tmp_path, *extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    with pytest.raises(SystemExit):
        _parse(tmp_path, "--fit", "--fit_refine", "bilateral")
    assert _parse(tmp_path, "--fit", "--fit_refine", "none", "--fit_radius", "0", "--fit_eps", "0").fit_refine == "none"      # unused: not looked at


def test_refine_arguments_of_the_library_path():
    from cfen_vit_dehazing_amd import fit
    fit.check_refine(None, 0, -1)                     # without refine, radius and eps are not looked at
    fit.check_refine("guided", 2, 1e-4)
    fit.check_refine("guided", np.int64(3), np.float32(1e-3))                 # anything int() and float() take
    fit.check_refine("guided", 2, torch.tensor(1e-4))
    for bad in (("guided", None, 1e-4), ("guided", float("nan"), 1e-4), ("guided", 2.5, 1e-4), ("guided", 2, None), ("guided", 2, "small")):
        with pytest.raises(ValueError, match="forward_fit: (radius|eps)"):
            fit.check_refine(*bad)
    for bad in (("bilateral", 2, 1e-4), ("guided", 0, 1e-4), ("guided", 17, 1e-4), ("guided", 2, 0.0), ("guided", 2, float("nan")), ("guided", 2, float("inf"))):
        with pytest.raises(ValueError, match="forward_fit"):
            fit.check_refine(*bad)


# ---- the new header's ledger ------------------------------------------------------------------------------------------------------------------------
def test_guided_header_is_exported_bound_and_apart_from_the_frozen_abi():
    cabi_ledger.check_header_bound("cfen_guided.h", {"cfen_guided_coef_u8": 10, "cfen_guided_apply_u8": 9})
