"""Motion compensation (include/cfen_motion.h) on the host: the numpy restatement tests/motion_ref.py against a plain loop, the exact properties of
the search (translations found, ties, the bias) and of the compensated recursion (a zero field, batching), the synthetic panning experiment
behind the defaults, the --temporal_mc options of dehaze_video.py, check_mc_params, the header's ledger and the argument
errors of the two entry points.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cabi_ledger
import motion_ref as ref
import temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the search -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,w,block,R,bias", [("random", 11, 13, 8, 2, 0), ("shift", 9, 19, 8, 3, 4), ("flat", 5, 7, 16, 2, 4),
                                                   ("border", 10, 12, 8, 5, 1)])
def test_the_vectorised_search_is_the_plain_loop(kind, h, w, block, R, bias):
    f = ref.frames(kind, h, w, 1, 5)
    vec, sad = ref.search_one(f[1], f[0], block, R, bias)
    want_vec, want_sad = ref.search_plain(f[1], f[0], block, R, bias)
    assert np.array_equal(vec, want_vec) and np.array_equal(sad, want_sad)
    assert vec.dtype == np.int16 and sad.dtype == np.int32 and vec.shape == (-(-h // block), -(-w // block), 2)


@pytest.mark.parametrize("block,R,bias", [(8, 3, 0), (16, 2, 4), (8, 2, 255)])
def test_every_translation_is_found_exactly(block, R, bias):
    """a random texture translated by every v with |dy|, |dx| <= R: every block whose search window lies inside the frame returns exactly v with
    sad == 0 (the SAD of random bytes at any other vector, about 85 levels per byte, is far above the largest bias, 16 levels per pixel)"""
    h, w = 4 * block, 5 * block
    rs = np.random.RandomState(block + R)
    base = rs.randint(0, 256, (h + 2 * R, w + 2 * R, 3), dtype=np.uint8)
    prv = base[R:R + h, R:R + w]
    bh, bw, _ = ref.grid(h, w, block)
    inner = np.zeros((bh, bw), bool)
    lo = -(-R // block)
    inner[lo:bh - lo, lo:bw - lo] = True                         # blocks at least R pixels from every edge
    assert inner.any()
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            cur = base[R + dy:R + dy + h, R + dx:R + dx + w]     # cur(p) = prv(p + v) wherever p + v lies inside the frame
            vec, sad = ref.search_one(cur, prv, block, R, bias)
            assert (vec[inner] == (dy, dx)).all() and not sad[inner].any(), (dy, dx)


@pytest.mark.parametrize("bias", [0, 4, 255])
def test_flat_and_identical_frames_return_zero(bias):
    """every candidate of a flat pair ties in SAD, every candidate of an identical pair is beaten or tied by SAD(0) = 0: the bias and then the
    shorter vector decide, for (0, 0)"""
    rs = np.random.RandomState(1)
    flat = np.broadcast_to(rs.randint(0, 256, (1, 1, 3), dtype=np.uint8), (19, 23, 3))
    other = np.broadcast_to(rs.randint(0, 256, (1, 1, 3), dtype=np.uint8), (19, 23, 3))
    same = rs.randint(0, 256, (19, 23, 3), dtype=np.uint8)
    for block in ref.BLOCKS:
        for cur, prv in ((flat, flat), (flat, other), (same, same)):
            vec, sad = ref.search_one(cur, prv, block, 3, bias)
            assert not vec.any()
            _, _, nb = ref.grid(19, 23, block)
            assert np.array_equal(sad, nb * int(np.abs(cur[0, 0].astype(int) - prv[0, 0]).sum()) if cur is flat else np.zeros_like(sad))


def test_ties_resolve_by_the_stated_order():
    """a pattern of period 2 along x matches equally at dx = -1 and +1 (and -2, 0, 2 not at all): equal cost and equal |v|_1, so the smaller
    (dy, dx) wins, (0, -1); vertically the same gives (-1, 0), which also beats (0, -1) on a checkerboard"""
    h, w = 24, 24
    y, x = np.mgrid[0:h, 0:w]
    for pattern, want in ((x % 2, (0, -1)), (y % 2, (-1, 0)), ((x + y) % 2, (-1, 0))):
        prv = np.repeat((pattern * 200)[:, :, None], 3, axis=2).astype(np.uint8)
        cur = 200 - prv                                          # the pattern moved by one pixel
        for bias in (0, 4):
            vec, sad = ref.search_one(cur, prv, 8, 2, bias)
            assert tuple(vec[1, 1]) == want and sad[1, 1] == 0, (want, bias, vec[1, 1])          # the block that no clamped border reaches


# ---- the compensated recursion ---------------------------------------------------------------------------------------------------------------------
def _clip(n=5, H=23, W=31, seed=2):
    rs = np.random.RandomState(seed)
    G = rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)
    G[2] = G[1]
    return G, rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("down", [1, 2])
def test_a_zero_field_is_the_uncompensated_run(down):
    G, Y = _clip()
    plain = temporal_ref.Stabiliser(down=down)
    zero = ref.Stabiliser(down=down, mc_block=8, field=lambda I, prev: np.zeros(ref.grid(I.shape[0], I.shape[1], 8)[:2] + (2,), np.int16))
    off = ref.Stabiliser(down=down)                              # mc_range = 0
    for k in range(len(G)):
        want = plain.step(G[k], Y[k])
        for st in (zero, off):
            got = st.step(G[k], Y[k])
            assert all(np.array_equal(a, b) for a, b in zip(got[:4], want)), k
            assert np.array_equal(st.state, plain.state)


def test_identical_hazy_frames_equal_the_uncompensated_run():
    """SAD(0) = 0 wins every tie, so the field is zero"""
    G, Y = _clip()
    G[:] = G[0]
    want, _ = ref.stabilise(G, Y)
    got, _ = ref.stabilise(G, Y, mc_range=4, mc_block=8, mc_bias=0)
    assert np.array_equal(got, want) and not np.array_equal(got, Y)


def test_the_restatement_does_not_depend_on_batching():
    """the device searches a batch in one launch; the restatement's batched search is frame by frame the one-frame search"""
    f = ref.frames("shift", 20, 27, 4, 3)
    vec, sad = ref.search(f[1:], f[0], 8, 3, 4)
    for k in range(4):
        v1, s1 = ref.search(f[k + 1:k + 2], f[k], 8, 3, 4)
        assert np.array_equal(v1[0], vec[k]) and np.array_equal(s1[0], sad[k])
    assert vec.any()


def test_warp():
    rs = np.random.RandomState(4)
    h, w, block = 13, 21, 8
    prev, state = rs.randint(0, 256, (h, w, 3), dtype=np.uint8), rs.normal(size=(h, w, 6)).astype(np.float32)
    vec = rs.randint(-16, 17, (2, 3, 2)).astype(np.int16)
    p, s = ref.warp(vec, prev, state, block)
    for y in range(h):
        for x in range(w):
            dy, dx = vec[y // block, x // block]
            sy, sx = min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)
            assert np.array_equal(p[y, x], prev[sy, sx]) and np.array_equal(s[y, x], state[sy, sx])
    p, s = ref.warp(np.zeros_like(vec), prev, state, block)
    assert np.array_equal(p, prev) and np.array_equal(s, state)


# ---- the experiment behind the defaults -----------------------------------------------------------------------------------------------------------
# the clip: motion_ref.PAN_SCENE, PAN_JITTER, PAN_STEP = (1, 3) pixels per frame, searched within +-PAN_RANGE = 4
# flicker along the motion (levels): the network's frames, --temporal alone, --temporal --temporal_mc 4 at the defaults; and the ratios to the first
PANNING = (8.186, 8.184, 1.403)
PANNING_RATIOS = (1.000, 0.171)
PANNING_PSNR = (31.714, 31.715, 36.172)          # dB against the clean frames, frames 4 onward, in the same order
ALONE_WITHIN = 0.02                  # --temporal alone stays within 2 % of the raw flicker on this clip: the recursion is switched off everywhere
# the same pan over a scene whose upper 40 % is a textureless sky, with sensor noise of 2 levels on every hazy frame: no match is exact
HARD = (8.276, 7.420, 4.407)
HARD_PSNR = (30.453, 30.876, 34.053)


def _panning(**kw):
    from cfen_vit_dehazing_amd import temporal
    G, Y, J, origin, alone, mc = ref.panning_case(temporal.MC_DEFAULTS["block"], temporal.MC_DEFAULTS["bias"], **kw)
    assert ref.flicker_along_motion(J, origin) == 0            # the measure is zero for the clean scene
    assert np.array_equal(mc[0], Y[0])                         # the first frame of a stream is the network's
    flick = [ref.flicker_along_motion(f, origin) for f in (Y, alone, mc)]
    psnr = [ref.psnr(f[4:], J[4:]) for f in (Y, alone, mc)]
    print("flicker along the motion: network %.3f, --temporal alone %.3f (%.3f), compensated %.3f (%.3f); PSNR %.3f, %.3f, %.3f dB"
          % (flick[0], flick[1], flick[1] / flick[0], flick[2], flick[2] / flick[0], psnr[0], psnr[1], psnr[2]))
    return flick, psnr


def test_a_panning_camera_flickers_less_with_compensation():
    """the static scene of section 18 (a), wider than the frame, under a window that moves (1, 3) pixels per frame; the same
    jittering 'network'.  Flicker is measured along the motion.  Three conditions: compensated < raw; --temporal alone within ALONE_WITHIN of raw
    (the defect: every pixel changed, the recursion is off); PSNR not below raw's by more than the margin, which is what --temporal alone moves the
    PSNR by in the same run (the resolution of this short clip).  The measured figures are pinned."""
    flick, psnr = _panning()
    raw, alone, mc = flick
    assert mc < raw
    assert abs(alone - raw) <= ALONE_WITHIN * raw
    margin = abs(psnr[1] - psnr[0])
    assert psnr[2] >= psnr[0] - margin
    assert np.allclose(flick, PANNING, atol=1e-3) and np.allclose([alone / raw, mc / raw], PANNING_RATIOS, atol=1e-3)
    assert np.allclose(psnr, PANNING_PSNR, atol=1e-3)


def test_a_panning_camera_over_sky_with_sensor_noise():
    """the harder clip the grid of DESIGN section 20 was run on: compensation still wins, by less (the noise itself keeps `keep` below 1)"""
    flick, psnr = _panning(sky=0.4, noise=2.0)
    assert flick[2] < flick[1] < flick[0] and psnr[2] >= psnr[0] - abs(psnr[1] - psnr[0])
    assert np.allclose(flick, HARD, atol=1e-3) and np.allclose(psnr, HARD_PSNR, atol=1e-3)


# ---- the --temporal_mc options at parsing -------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    return VideoOptions().parse(["--in", "clip.y4m", "--out", str(tmp_path / "out.y4m"), "--name", "video", "--gpu_ids", "-1",
                                 "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_temporal_mc_flags_and_refusals(tmp_path, capsys):
    from cfen_vit_dehazing_amd import temporal
    assert temporal.MC_DEFAULTS == {"range": 0, "block": 16, "bias": 4}
    for args in ((), ("--temporal",), ("--temporal", "--temporal_mc", "0")):
        opt = _parse(tmp_path, *args)
        text = capsys.readouterr().out
        assert "\ntemporal_mc" not in text and "video_matrix: auto" in text          # a run without the flag prints and records what it always did
        assert "\ntemporal_mc" not in open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
        assert ("temporal_strength: 0.8" in text) == bool(args)
        assert not getattr(opt, "temporal_mc", None)
    opt = _parse(tmp_path, "--temporal", "--temporal_mc", "8")
    assert (opt.temporal_mc, opt.temporal_mc_block, opt.temporal_mc_bias) == (8, 16, 4)
    text = capsys.readouterr().out
    assert all(l in text for l in ("temporal_mc: 8", "temporal_mc_block: 16", "temporal_mc_bias: 4", "temporal: True"))
    assert "temporal_mc_block: 16" in open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
    opt = _parse(tmp_path, "--temporal", "--temporal_mc", "16", "--temporal_mc_block", "32", "--temporal_mc_bias", "255", "--fit", "--eval_noref")
    assert (opt.temporal_mc, opt.temporal_mc_block, opt.temporal_mc_bias) == (16, 32, 255)
    capsys.readouterr()
    for flag, value in (("--temporal_mc", "4"), ("--temporal_mc_block", "8"), ("--temporal_mc_bias", "2")):
        with pytest.raises(ValueError) as e:                                          # each of the three needs --temporal
            _parse(tmp_path, flag, value)
        assert flag in str(e.value) and "--temporal" in str(e.value).replace(flag, ""), str(e.value)
    for extra in (("--temporal_mc_block", "8"), ("--temporal_mc_bias", "2"), ("--temporal_mc", "0", "--temporal_mc_bias", "2")):
        with pytest.raises(ValueError) as e:                                          # the last two need --temporal_mc > 0
            _parse(tmp_path, "--temporal", *extra)
        assert extra[-2] in str(e.value) and "--temporal_mc > 0" in str(e.value), str(e.value)
    for flag, values in (("--temporal_mc", ("-1", "17")), ("--temporal_mc_bias", ("-1", "256"))):
        for v in values:
            with pytest.raises(ValueError) as e:
                _parse(tmp_path, "--temporal", "--temporal_mc", "4", "%s=%s" % (flag, v))
            assert flag + " must be" in str(e.value), (flag, v, str(e.value))
    for extra in (("--temporal_mc_block", "12"), ("--temporal_mc", "2.5"), ("--temporal_mc_bias", "x")):
        with pytest.raises(SystemExit) as e:                                          # what argparse itself refuses leaves with 2 as well
            _parse(tmp_path, "--temporal", "--temporal_mc", "4", *extra)
        assert e.value.code == 2
        assert extra[0] in capsys.readouterr().err


def test_the_help_text_says_where_the_mc_defaults_come_from():
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    o = VideoOptions()
    o.initialize()
    text = " ".join(o.parser.format_help().split())
    tail = text.split("--temporal_mc_bias TEMPORAL_MC_BIAS")[-1]
    assert "synthetic panning experiment" in tail and "not from a checkpoint" in tail


def test_check_mc_params():
    from cfen_vit_dehazing_amd import temporal
    assert temporal.check_mc_params(0, 16, 4) == (0, 16, 4)
    assert temporal.check_mc_params(np.int64(16), np.int32(8), 255.0) == (16, 8, 255)
    for bad, name in (((-1, 16, 4), "mc_range"), ((17, 16, 4), "mc_range"), ((2.5, 16, 4), "mc_range"), ((None, 16, 4), "mc_range"),
                      ((4, 12, 4), "mc_block"), ((4, 0, 4), "mc_block"), ((4, "16", 4), "mc_block"), ((4, 16, -1), "mc_bias"), ((4, 16, 256), "mc_bias"),
                      ((4, 16, 0.5), "mc_bias")):
        with pytest.raises(ValueError, match="Stabiliser: %s must be" % name):
            temporal.Stabiliser(mc_range=bad[0], mc_block=bad[1], mc_bias=bad[2])
    with pytest.raises(TypeError):
        temporal.Stabiliser(2, 1e-4, 0.8, 8.0, "auto", 4)                             # the new arguments are keyword-only
    st = temporal.Stabiliser(mc_range=4)
    assert (st.mc_range, st.mc_block, st.mc_bias) == (4, 16, 4) and temporal.Stabiliser().mc_range == 0


# ---- the new header's ledger ------------------------------------------------------------------------------------------------------------------------
def test_motion_header_is_exported_bound_and_apart_from_the_older_tables():
    fns = {"cfen_motion_search_u8": 11, "cfen_motion_warp": 9}
    cabi_ledger.check_header_bound("cfen_motion.h", fns, word="motion_search")
    cabi_ledger.check_guard_band_test_calls("test_hip_motion.py", "test_guard_bands_motion", fns)


def test_the_definition_stands_in_the_header():
    text = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "cfen_motion.h")).read()).split())
    for phrase in ("SAD(v) = sum_{p in block} sum_c |I_t(p, c) - I_{t-1}(clamp(p + v), c)|", "cost(v) = 16 * SAD(v) + bias * (|dy| + |dx|) * 3 * n_b",
                   "lexicographically smallest (cost, |dy| + |dx|, dy, dx)", "prev_out(p) = prev_guide(clamp(p + v_b))",
                   "state_out(p, 0..5) = state(clamp(p + v_b), 0..5)", "a zero vector field makes the warp a copy",
                   "does not depend on how frames are grouped into batches", "Bk in {8, 16, 32}", "R in 1 .. 16"):
        assert phrase in text, phrase


# ---- the C entry points refuse bad arguments before any launch --------------------------------------------------------------------------------------
def test_motion_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    g, p, v, s, st, po, so, z = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6, 7, 0))      # never dereferenced
    refused, off = functools.partial(cabi_ledger.refused, lib), cabi_ledger.off

    for bad in ((z, p, v, s), (g, z, v, s), (g, p, z, s), (g, p, v, z)):
        refused("motion_search_u8", b"null pointer", bad[0], bad[1], 1, 20, 20, 8, 2, 4, bad[2], bad[3], z)
    refused("motion_search_u8", b"B = 0", g, p, 0, 20, 20, 8, 2, 4, v, s, z)
    refused("motion_search_u8", b"B = 65537", g, p, 65537, 20, 20, 8, 2, 4, v, s, z)
    refused("motion_search_u8", b"h = 0", g, p, 1, 0, 20, 8, 2, 4, v, s, z)
    refused("motion_search_u8", b"w = 16385", g, p, 1, 20, 16385, 8, 2, 4, v, s, z)
    for block in (0, 4, 12, 64, -8):
        refused("motion_search_u8", b"block = %d" % block, g, p, 1, 20, 20, block, 2, 4, v, s, z)
    refused("motion_search_u8", b"range = 0", g, p, 1, 20, 20, 8, 0, 4, v, s, z)
    refused("motion_search_u8", b"range = 17", g, p, 1, 20, 20, 8, 17, 4, v, s, z)
    refused("motion_search_u8", b"bias = -1", g, p, 1, 20, 20, 8, 2, -1, v, s, z)
    refused("motion_search_u8", b"bias = 256", g, p, 1, 20, 20, 8, 2, 256, v, s, z)
    for bad in ((off(v, 2), s), (v, off(s, 1)), (off(v, 1), s)):
        refused("motion_search_u8", b"4-byte aligned", g, p, 1, 20, 20, 8, 2, 4, bad[0], bad[1], z)
    # B = 2 frames of 20 x 20: guide 2400 bytes, prev_guide 1200, vec and sad 2 * 9 * 4 = 72
    for bad in ((g, g, v, s), (g, off(g, 2399), v, s), (g, p, v, v), (g, p, v, off(v, 68)), (g, p, g, s), (g, p, v, off(p, 1196)), (g, off(g, -1199), v, s)):
        refused("motion_search_u8", b"must not overlap", bad[0], bad[1], 2, 20, 20, 8, 2, 4, bad[2], bad[3], z)

    for bad in ((z, p, st, po, so), (v, z, st, po, so), (v, p, z, po, so), (v, p, st, z, so), (v, p, st, po, z)):
        refused("motion_warp", b"null pointer", bad[0], bad[1], bad[2], 20, 20, 8, bad[3], bad[4], z)
    refused("motion_warp", b"h = 0", v, p, st, 0, 20, 8, po, so, z)
    refused("motion_warp", b"w = 16385", v, p, st, 20, 16385, 8, po, so, z)
    for block in (0, 12, 64):
        refused("motion_warp", b"block = %d" % block, v, p, st, 20, 20, block, po, so, z)
    refused("motion_warp", b"4-byte aligned", off(v, 2), p, st, 20, 20, 8, po, so, z)
    for bad in ((off(st, 8), so), (st, off(so, 4))):
        refused("motion_warp", b"16-byte aligned", v, p, bad[0], 20, 20, 8, po, bad[1], z)
    # 20 x 20: vec 36 bytes, prev_guide and prev_out 1200, state and state_out 9600
    for bad in ((v, p, st, p, so), (v, p, st, po, st), (v, p, st, off(p, 1199), so), (v, p, st, po, off(st, 9584)), (v, p, st, off(v, 35), so),
                (v, p, st, po, off(po, 1184)), (v, off(st, 9599), st, po, so)):
        refused("motion_warp", b"must not overlap", bad[0], bad[1], bad[2], 20, 20, 8, bad[3], bad[4], z)
