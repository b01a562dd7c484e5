"""Temporal stabilisation (include/cfen_temporal.h) on the host: the three exact consequences of the definition on the numpy restatement
tests/temporal_ref.py, the tolerance TAU_T of tests/test_hip_temporal.py, the synthetic experiment behind the defaults, the
argument errors of the two entry points, the --temporal options of dehaze_video.py, and the header's ledger.  No GPU."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import cabi_ledger
import guided_ref
import temporal_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tolerance of tests/test_hip_temporal.py: 8 x the largest |x_float32 - x_float64| over every case of that file, where x is Delta and the state S
# of a blend case (the recursion over the B frames included) and the pre-rounding value v of an apply case, and float32 is the header's formulas
# rounded to fp32 step by step on the CPU (temporal_ref, dtype=float32) -- never the kernels.  The factor 8 is for fused multiply-adds.
# Measured: 6.002e-5 (a blend case: offsets of up to 300 levels, whose fp32 spacing is 3.05e-5); the apply cases reach 3.004e-5.  test_tau recomputes it.
TAU_T = 4.80e-4


# ---- the three exact consequences ---------------------------------------------------------------------------------------------------------------------
def _pair(seed, H=23, W=31):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (H, W, 3), dtype=np.uint8), rs.randint(0, 256, (H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("down", [1, 2])
def test_identical_frames_pass_unchanged(dtype, down):
    G, Y = _pair(1)
    st = ref.Stabiliser(down=down, dtype=dtype)
    for _ in range(3):
        dst, v, delta, keep = st.step(G, Y)
        assert not delta.any() and np.array_equal(dst, Y) and np.array_equal(v, Y.astype(dtype))
    assert (keep == 1).all()                                   # the recursion was on, and had nothing to change


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_cut_passes_unchanged(dtype):
    st = ref.Stabiliser(dtype=dtype)
    G0, Y0 = _pair(2)
    st.step(G0, Y0)
    G1 = (G0.astype(np.int64) + 100).astype(np.uint8)          # every byte moves by 100 or 156 levels: d >= motion everywhere
    Y1 = _pair(3)[1]
    dst, v, delta, keep = st.step(G1, Y1)
    assert not keep.any() and not delta.any() and np.array_equal(dst, Y1)
    a, b = guided_ref.smoothed(G1, Y1, 2, 1e-4, dtype)
    assert np.array_equal(st.state, np.concatenate([a, b], axis=2).astype(np.float32).astype(dtype))          # S_t = c_t


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_strength_zero_passes_every_input_unchanged(dtype):
    st = ref.Stabiliser(strength=0.0, dtype=dtype)
    for seed in range(4, 8):
        G, Y = _pair(seed)
        if seed == 6:
            G = st.prev                                        # also where keep is 1
        dst, v, delta, keep = st.step(G, Y)
        assert not delta.any() and np.array_equal(dst, Y)


def test_the_recursion_is_an_exponential_average_where_nothing_moves():
    """a static guide and constant-per-frame outputs: keep = 1, and S follows c with weight strength, so the correction is the smoothed offset"""
    G = _pair(8)[0]
    st = ref.Stabiliser(strength=0.5)
    S = None
    for level in (100, 120, 90, 140):
        Y = np.full_like(G, level)
        dst, v, delta, keep = st.step(G, Y)
        assert (keep == (0 if S is None else 1)).all()             # (keep of a stream's first frame is 0 by the restatement's convention)
        S = level if S is None else level + np.float64(np.float32(0.5)) * (S - level)
        assert np.abs(delta[..., :3]).max() == 0 and np.abs(delta[..., 3:] - (S - level)).max() <= 1e-9
        assert np.array_equal(dst, ref.to_bytes(np.full(G.shape, S)))


def test_working_size():
    assert ref.working_size(512, 512) == (1, 512, 512) and ref.working_size(1024, 600) == (1, 1024, 600)
    assert ref.working_size(1025, 600) == (2, 513, 300) and ref.working_size(2160, 3840) == (4, 540, 960) and ref.working_size(150, 201, 4) == (4, 38, 51)
    from cfen_vit_dehazing_amd import temporal
    for args in ((512, 512), (1025, 600), (2160, 3840), (150, 201, 4), (7, 9, 1)):
        assert temporal.working_size(*args) == ref.working_size(*args)


# ---- the tolerance ---------------------------------------------------------------------------------------------------------------------------------
def test_tau():
    worst = {}
    for h, w in ref.SIZES:
        for r in ref.RADII:
            for B in ref.BATCHES:
                for have in (False, True):
                    guide, prev, coef, state0, delta64, state64, _, _ = ref.blend_case(h, w, r, B, have)
                    delta32, state32, _, _ = ref.blend(guide, prev if have else None, coef, r, ref.MOTION, ref.STRENGTH, state0, np.float32)
                    assert delta32.dtype == np.float32 and state32.dtype == np.float32
                    d = max(np.abs(delta32.astype(np.float64) - delta64).max(), np.abs(state32.astype(np.float64) - state64).max())
                    worst["blend %dx%d r%d B%d %d" % (h, w, r, B, have)] = float(d)
    for name in ref.APPLY_CASES:
        delta, G, Y, v64 = ref.apply_case(name)
        v32 = ref.apply_v(delta[0], G[0], Y[0], np.float32)
        worst["apply " + name] = float(np.abs(v32.astype(np.float64) - v64[0]).max())
    top = max(worst.values())
    print("max |x32 - x64| = %.4e (%s); apply cases %.4e; TAU_T = %.3e = %.2f x"
          % (top, max(worst, key=worst.get), max(v for k, v in worst.items() if k.startswith("apply")), TAU_T, TAU_T / top))
    assert 4 * top <= TAU_T <= 16 * top


# ---- the experiment behind the defaults -----------------------------------------------------------------------------------------------------------
SCENE = (96, 128, 12, 3)             # H, W, frames, seed
JITTER = (6.0, 0.04)                 # standard deviation of the assumed airlight (levels) and of the assumed transmission (relative), per frame
STATIC = (8.300, 1.395, 0.168)       # flicker of the network's frames and of the stabilised ones (levels), and their ratio
MOVING = (29.935, 29.936)            # PSNR inside the moving object's footprint: unstabilised, stabilised (dB)
MOVING_MARGIN = 0.05                 # dB, see test_a_moving_object_and_a_cut


def _run(G, Y):
    st = ref.Stabiliser()
    return [st.step(G[k], Y[k]) for k in range(len(G))]


def test_static_scene_flickers_less():
    """the scattering-model scene of section 14, static, 12 frames; the 'network' is the ideal dehazer whose guess of the
    airlight and of the transmission jitters from frame to frame, independently.  Flicker = mean |out_t - out_{t-1}| over frames 4 onward.  For
    independent jitter an exponential average with weight 0.8 brings frame-to-frame differences down to (1 - 0.8) / sqrt(1 + 0.8) = 0.149 of the
    raw ones; the bound 0.30 leaves a factor 2 for the short sequence, the byte rounding and the fit.  The measured figures are pinned."""
    H, W, n, seed = SCENE
    G, Y, J, _ = ref.jitter_stream(H, W, n, seed, *JITTER)
    assert (G == G[0]).all()
    out = np.stack([r[0] for r in _run(G, Y)])
    raw, stab = ref.flicker(Y), ref.flicker(out)
    print("flicker: network %.3f levels, stabilised %.3f, ratio %.3f; PSNR against the clear scene %.2f -> %.2f dB"
          % (raw, stab, stab / raw, ref.psnr(Y[4:], J[4:]), ref.psnr(out[4:], J[4:])))
    assert np.array_equal(out[0], Y[0])                        # the first frame of a stream is the network's
    assert stab <= 0.30 * raw
    assert np.allclose([raw, stab, stab / raw], STATIC, atol=1e-3)


def test_a_moving_object_and_a_cut():
    """the same scene with a textured object crossing it, 3 pixels a frame, and a cut to another scene at frame 6.  The frame
    after the cut is the network's, byte for byte.  Inside the object's footprint the motion test switches the recursion off (keep averages under
    0.01 there), so the bytes are almost all the network's: measured, the PSNR against the clear frame inside the footprint is 29.935 dB without
    and 29.936 dB with stabilisation.  The margin: the two figures are pinned to 0.01 dB, and 0.05 dB (1.2 % of the mean squared error, five times
    the pin) is the smallest loss this short sequence could tell from nothing; a stabiliser that ghosts moving objects loses whole dB there."""
    H, W, n, seed = SCENE
    G, Y, J, F = ref.jitter_stream(H, W, n, seed, *JITTER, moving=True, cut_at=6)
    res = _run(G, Y)
    out = np.stack([r[0] for r in res])
    assert not res[6][3].any() and np.array_equal(out[6], Y[6]) and not np.array_equal(out[5], Y[5]) and not np.array_equal(out[7], Y[7])
    sel = F.copy()
    sel[0] = False                                             # frame 0 has no predecessor
    raw, stab = ref.psnr(Y[sel], J[sel]), ref.psnr(out[sel], J[sel])
    keep = np.mean([res[k][3][F[k]].mean() for k in range(1, n)])
    print("inside the footprint: %.3f dB unstabilised, %.3f dB stabilised, mean keep %.4f; outside: %.2f -> %.2f dB"
          % (raw, stab, keep, ref.psnr(Y[~F], J[~F]), ref.psnr(out[~F], J[~F])))
    assert stab >= raw - MOVING_MARGIN
    assert np.allclose([raw, stab], MOVING, atol=0.01) and keep < 0.01


# ---- the C entry points refuse bad arguments before any launch --------------------------------------------------------------------------------------
def test_temporal_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    g, p, c, s, d, hi, src, dst, z = (ctypes.c_void_p(v << 20) for v in (1, 2, 3, 4, 5, 6, 7, 8, 0))      # never dereferenced
    f = ctypes.c_float
    refused, off = functools.partial(cabi_ledger.refused, lib), cabi_ledger.off

    for bad in ((z, p, c, s, d), (g, z, c, s, d), (g, p, z, s, d), (g, p, c, z, d), (g, p, c, s, z)):
        refused("temporal_blend", b"null pointer", bad[0], bad[1], bad[2], 1, 4, 4, 2, f(8), f(0.8), 1, bad[3], bad[4], z)
    refused("temporal_blend", b"null pointer", g, z, c, 1, 4, 4, 2, f(8), f(0.8), 0, z, d, z)          # without state prev_guide may be null, state not
    refused("temporal_blend", b"have_state = 2", g, p, c, 1, 4, 4, 2, f(8), f(0.8), 2, s, d, z)
    refused("temporal_blend", b"B = 0", g, p, c, 0, 4, 4, 2, f(8), f(0.8), 1, s, d, z)
    refused("temporal_blend", b"B = 65537", g, p, c, 65537, 4, 4, 2, f(8), f(0.8), 1, s, d, z)
    refused("temporal_blend", b"h = 0", g, p, c, 1, 0, 4, 2, f(8), f(0.8), 1, s, d, z)
    refused("temporal_blend", b"w = 16385", g, p, c, 1, 4, 16385, 2, f(8), f(0.8), 1, s, d, z)
    refused("temporal_blend", b"radius = 0", g, p, c, 1, 4, 4, 0, f(8), f(0.8), 1, s, d, z)
    refused("temporal_blend", b"radius = 17", g, p, c, 1, 4, 4, 17, f(8), f(0.8), 1, s, d, z)
    for motion in (0.0, -1.0, math.nan, math.inf):
        refused("temporal_blend", b"motion", g, p, c, 1, 4, 4, 2, f(motion), f(0.8), 1, s, d, z)
    for strength in (-0.1, 1.0, 1.5, math.nan, math.inf):
        refused("temporal_blend", b"strength", g, p, c, 1, 4, 4, 2, f(8), f(strength), 1, s, d, z)
    for bad in ((off(c, 4), s, d), (c, off(s, 8), d), (c, s, off(d, 4))):
        refused("temporal_blend", b"16-byte aligned", g, p, bad[0], 1, 4, 4, 2, f(8), f(0.8), 1, bad[1], bad[2], z)
    for bad in ((g, g, c, s, d), (g, p, c, s, c), (g, p, c, s, s), (g, p, s, s, d), (g, off(g, 47), c, s, d), (g, p, c, s, off(c, 368)),
                (g, p, c, off(d, 384 * 2 - 16), d)):                                         # B = 2 frames of 4 x 4: coef and delta are 768 bytes
        refused("temporal_blend", b"must not overlap", bad[0], bad[1], bad[2], 2, 4, 4, 2, f(8), f(0.8), 1, bad[3], bad[4], z)

    for bad in ((z, hi, src, dst), (d, z, src, dst), (d, hi, z, dst), (d, hi, src, z)):
        refused("temporal_apply_u8", b"null pointer", bad[0], 1, 4, 4, bad[1], bad[2], 8, 8, bad[3], z)
    refused("temporal_apply_u8", b"B = 0", d, 0, 4, 4, hi, src, 8, 8, dst, z)
    refused("temporal_apply_u8", b"w = 0", d, 1, 4, 0, hi, src, 8, 8, dst, z)
    refused("temporal_apply_u8", b"H = 0", d, 1, 4, 4, hi, src, 0, 8, dst, z)
    refused("temporal_apply_u8", b"W = 16385", d, 1, 4, 4, hi, src, 8, 16385, dst, z)
    refused("temporal_apply_u8", b"h = 16385", d, 1, 16385, 4, hi, src, 8, 8, dst, z)
    refused("temporal_apply_u8", b"16-byte aligned", off(d, 8), 1, 4, 4, hi, src, 8, 8, dst, z)
    for bad in ((d, hi, src, hi), (d, hi, src, src), (d, hi, hi, dst), (d, hi, src, d), (d, d, src, dst), (d, hi, src, off(src, 191)),
                (d, hi, src, off(hi, -191))):
        refused("temporal_apply_u8", b"must not overlap", bad[0], 1, 4, 4, bad[1], bad[2], 8, 8, bad[3], z)


# ---- the --temporal options at parsing ------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    return VideoOptions().parse(["--in", "clip.y4m", "--out", str(tmp_path / "out.y4m"), "--name", "video", "--gpu_ids", "-1",
                                 "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_temporal_flags_and_refusals(tmp_path, capsys):
    opt = _parse(tmp_path)
    assert opt.temporal is False
    text = capsys.readouterr().out
    assert "\ntemporal" not in text and "video_matrix: auto" in text                 # a run without the flag prints and records what it always did
    assert "\ntemporal" not in open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
    opt = _parse(tmp_path, "--temporal")
    assert (opt.temporal, opt.temporal_strength, opt.temporal_motion, opt.temporal_radius, opt.temporal_eps, opt.temporal_down) == \
        (True, 0.8, 8.0, 2, 1e-4, "auto")
    text = capsys.readouterr().out
    assert all(l in text for l in ("temporal: True", "temporal_strength: 0.8", "temporal_motion: 8.0", "temporal_radius: 2", "temporal_eps: 0.0001",
                                   "temporal_down: auto"))
    opt = _parse(tmp_path, "--temporal", "--temporal_strength", "0", "--temporal_motion", "2.5", "--temporal_radius", "16", "--temporal_eps", "0.01",
                 "--temporal_down", "3", "--fit", "--eval_noref", "--batchSize", "2")
    assert (opt.temporal_strength, opt.temporal_motion, opt.temporal_radius, opt.temporal_eps, opt.temporal_down) == (0.0, 2.5, 16, 0.01, 3)
    capsys.readouterr()
    for flag, value in (("--temporal_strength", "0.5"), ("--temporal_motion", "4"), ("--temporal_radius", "3"), ("--temporal_eps", "1e-3"),
                        ("--temporal_down", "2"), ("--temporal_down", "auto")):
        with pytest.raises(ValueError) as e:                                          # each of the five needs --temporal
            _parse(tmp_path, flag, value)
        assert flag in str(e.value) and "--temporal" in str(e.value).replace(flag, ""), str(e.value)
    for flag, values in (("--temporal_strength", ("1", "1.5", "-0.1", "nan", "inf")), ("--temporal_motion", ("0", "-1", "nan", "inf")),
                         ("--temporal_radius", ("0", "17", "-2")), ("--temporal_eps", ("0", "-1e-4", "nan", "inf")),
                         ("--temporal_down", ("0", "-1", "1.5", "half"))):
        for v in values:
            with pytest.raises(ValueError) as e:
                _parse(tmp_path, "--temporal", "%s=%s" % (flag, v))
            assert flag in str(e.value), (flag, v, str(e.value))
    with pytest.raises(SystemExit) as e:                                              # what argparse itself refuses leaves with 2 as well
        _parse(tmp_path, "--temporal", "--temporal_radius", "2.5")
    assert e.value.code == 2
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    capsys.readouterr()
    opt = TestOptions().parse(["--dataroot", str(tmp_path), "--name", "video", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path / "ckpt"), "--temporal"])
    assert not hasattr(opt, "temporal")                                               # test.py does not get the flag: to it, it is one it does not know
    assert "ignoring flags outside the inference path: --temporal" in capsys.readouterr().out


def test_the_help_text_says_where_the_defaults_come_from():
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    o = VideoOptions()
    o.initialize()
    text = " ".join(o.parser.format_help().split())
    assert "not from a checkpoint" in text.split("--temporal_motion TEMPORAL_MOTION")[-1].split("--temporal_radius TEMPORAL_RADIUS")[0]


def test_stabiliser_arguments():
    from cfen_vit_dehazing_amd import temporal
    assert temporal.check_params(2, 1e-4, 0.8, 8.0, "auto") == (2, 1e-4, 0.8, 8.0, "auto")
    assert temporal.check_params(np.int64(3), np.float32(0.5), 0, 1, 4) == (3, 0.5, 0.0, 1.0, 4)
    for bad in ((0, 1e-4, 0.8, 8.0, "auto"), (17, 1e-4, 0.8, 8.0, "auto"), (2.5, 1e-4, 0.8, 8.0, "auto"), (2, 0.0, 0.8, 8.0, "auto"),
                (2, math.nan, 0.8, 8.0, "auto"), (2, 1e-4, 1.0, 8.0, "auto"), (2, 1e-4, -0.1, 8.0, "auto"), (2, 1e-4, math.nan, 8.0, "auto"),
                (2, 1e-4, 0.8, 0.0, "auto"), (2, 1e-4, 0.8, math.inf, "auto"), (2, 1e-4, 0.8, 8.0, 0), (2, 1e-4, 0.8, 8.0, 1.5),
                (2, 1e-4, 0.8, 8.0, "twice"), (None, 1e-4, 0.8, 8.0, "auto")):
        with pytest.raises(ValueError, match="Stabiliser: (radius|eps|strength|motion|down)"):
            temporal.Stabiliser(*bad)
    assert temporal.DEFAULTS == {"radius": 2, "eps": 1e-4, "strength": 0.8, "motion": 8.0, "down": "auto"}


# ---- the new header's ledger ------------------------------------------------------------------------------------------------------------------------
def test_temporal_header_is_exported_bound_and_apart_from_the_older_tables():
    fns = {"cfen_temporal_blend": 13, "cfen_temporal_apply_u8": 10}
    cabi_ledger.check_header_bound("cfen_temporal.h", fns)
    cabi_ledger.check_guard_band_test_calls("test_hip_temporal.py", "test_guard_bands_temporal", fns)


def test_the_definition_stands_in_the_header():
    text = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "cfen_temporal.h")).read()).split())
    for phrase in ("S_t = c_t + k * (S_{t-1} - c_t)", "Delta_t = S_t - c_t", "keep = clamp(1 - d / motion, 0, 1)", "k = strength * keep",
                   "d = float(D) / float(3 N)", "v = (float(Y_t) + DA * G_t) + DB", "dst = uint8(clamp(floor(v + 0.5), 0, 255))"):
        assert phrase in text, phrase
