"""Sub-pixel motion compensation (include/cfen_subpel.h) on the host: the numpy restatement tests/subpel_ref.py against a plain loop, the exact
properties of the sample, the refinement and the warp (multiples of 4, ties, identical frames, batching), the synthetic panning experiment
behind the flag, the --temporal_mc_subpel option of dehaze_video.py, check_mc_subpel, the header's ledger and the argument
errors of the two entry points.  No GPU."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import cabi_ledger
import motion_ref
import subpel_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the sample and the refinement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", ref.BIASES)
@pytest.mark.parametrize("Q", ref.SUBPELS)
@pytest.mark.parametrize("h,w", motion_ref.SIZES)
def test_the_vectorised_refinement_is_the_plain_loop(h, w, Q, bias):
    for kind, block in (("subshift", 8), ("border", 16)):
        f = ref.frames(kind, h, w, 1, Q, 5)
        vec = motion_ref.search_one(f[1], f[0], block, 3, bias)[0]
        vec4, sad4 = ref.refine_one(f[1], f[0], vec, block, Q, bias)
        want_vec4, want_sad4 = ref.refine_plain(f[1], f[0], vec, block, Q, bias)
        assert np.array_equal(vec4, want_vec4) and np.array_equal(sad4, want_sad4), kind
        assert vec4.dtype == np.int16 and sad4.dtype == np.int32 and vec4.shape == vec.shape
        assert (np.abs(vec4.astype(int) - 4 * vec) <= 3).all() and not ((vec4.astype(int) - 4 * vec) % (4 // Q)).any()


def test_the_sample_at_multiples_of_four_is_the_pixel_and_lies_between_its_taps():
    rs = np.random.RandomState(1)
    img = rs.randint(0, 256, (9, 11, 3), dtype=np.uint8)
    y, x = np.mgrid[-3:12, -3:14]
    assert np.array_equal(ref.sample(img, 4 * y, 4 * x), img[np.clip(y, 0, 8), np.clip(x, 0, 10)])
    for fy in range(4):
        for fx in range(4):
            s = ref.sample(img, 4 * y + fy, 4 * x + fx)
            t = np.stack([img[np.clip(y + a, 0, 8), np.clip(x + b, 0, 10)].astype(np.int64) for a in (0, 1) for b in (0, 1)])
            assert (s >= t.min(axis=0)).all() and (s <= t.max(axis=0)).all()
    flat = np.full((5, 6, 3), 77, np.uint8)
    y, x = np.mgrid[-9:29, -9:33]
    assert (ref.sample(flat, y, x) == 77).all()                  # the weights sum to 16 at every fraction


@pytest.mark.parametrize("block", ref.BLOCKS)
def test_a_warp_by_multiples_of_four_is_the_whole_pixel_warp(block):
    rs = np.random.RandomState(block)
    h, w = 19, 37
    bh, bw, _ = ref.grid(h, w, block)
    prev, state = rs.randint(0, 256, (h, w, 3), dtype=np.uint8), rs.normal(0, 100, (h, w, 6)).astype(np.float32)
    vec = rs.randint(-16, 17, (bh, bw, 2)).astype(np.int16)
    want_p, want_s = motion_ref.warp(vec, prev, state, block)
    for dtype in (np.float64, np.float32):
        got_p, got_s = ref.warp((4 * vec).astype(np.int16), prev, state, block, dtype)
        assert got_p.dtype == np.uint8 and np.array_equal(got_p, want_p) and np.array_equal(got_s, want_s)
    got_p, got_s = ref.warp((4 * vec + 1).astype(np.int16), prev, state, block)
    assert not np.array_equal(got_p, want_p) and not np.array_equal(got_s, want_s)


def test_warp_by_a_loop_over_pixels():
    rs = np.random.RandomState(4)
    h, w, block = 13, 21, 8
    prev, state = rs.randint(0, 256, (h, w, 3), dtype=np.uint8), rs.normal(size=(h, w, 6))
    vec4 = rs.randint(-70, 71, (2, 3, 2)).astype(np.int16)
    p, s = ref.warp(vec4, prev, state, block)
    cl = lambda v, n: min(max(v, 0), n - 1)
    for y in range(h):
        for x in range(w):
            y4, x4 = 4 * y + int(vec4[y // block, x // block, 0]), 4 * x + int(vec4[y // block, x // block, 1])
            ya, yb, xa, xb = cl(y4 >> 2, h), cl((y4 >> 2) + 1, h), cl(x4 >> 2, w), cl((x4 >> 2) + 1, w)
            fy, fx = (y4 & 3) / 4, (x4 & 3) / 4
            t0 = state[ya, xa] + fx * (state[ya, xb] - state[ya, xa])
            t1 = state[yb, xa] + fx * (state[yb, xb] - state[yb, xa])
            assert np.array_equal(s[y, x], t0 + fy * (t1 - t0))
            assert np.array_equal(p[y, x], ref.sample(prev, np.array(y4), np.array(x4)))


@pytest.mark.parametrize("Q", ref.SUBPELS)
def test_refinement_never_raises_the_sad_without_a_bias(Q):
    """the whole-pixel winner is among the candidates, at 4 x its cost"""
    for kind in ("random", "subshift", "border"):
        f = ref.frames(kind, 40, 50, 2, Q, 7)
        vec, sad = motion_ref.search(f[1:], f[0], 8, 3, 0)
        vec4, sad4 = ref.refine(f[1:], f[0], vec, 8, Q, 0)
        assert (sad4 <= sad).all(), kind
        stays = (vec4 == 4 * vec).all(axis=-1)
        assert np.array_equal(sad4[stays], sad[stays])


@pytest.mark.parametrize("Q", ref.SUBPELS)
@pytest.mark.parametrize("h,w", [(17, 33), (40, 50)])
def test_the_subshift_inputs_give_fractional_fields(h, w, Q):
    """what the new input kind is for: at least half of the blocks end on a vector that is not whole.  A field that comes out whole would mean
    that the device tests on it test nothing"""
    for block in (8, 16):
        _, _, vec, vec4, _ = ref.refine_case("subshift", h, w, block, Q, 4, 3)
        share = ref.fractional_share(vec4)
        print("subshift %d x %d, block %d, Q %d: %.2f of the blocks fractional" % (h, w, block, Q, share))
        assert share >= 0.5
        assert not ((vec4.astype(int) - 4 * vec) % (4 // Q)).any()


@pytest.mark.parametrize("bias", [0, 4, 255])
def test_flat_and_identical_frames_return_zero(bias):
    """every candidate of a flat pair ties in SAD4, every candidate of an identical pair is beaten or tied by SAD4(0) = 0: the bias and then the
    shorter vector decide, for (0, 0)"""
    rs = np.random.RandomState(1)
    flat = np.broadcast_to(rs.randint(0, 256, (1, 1, 3), dtype=np.uint8), (19, 23, 3))
    other = np.broadcast_to(rs.randint(0, 256, (1, 1, 3), dtype=np.uint8), (19, 23, 3))
    same = rs.randint(0, 256, (19, 23, 3), dtype=np.uint8)
    for block in ref.BLOCKS:
        _, _, nb = ref.grid(19, 23, block)
        for Q in ref.SUBPELS:
            for cur, prv in ((flat, flat), (flat, other), (same, same)):
                vec = motion_ref.search_one(cur, prv, block, 3, bias)[0]
                vec4, sad4 = ref.refine_one(cur, prv, vec, block, Q, bias)
                assert not vec.any() and not vec4.any()
                assert np.array_equal(sad4, nb * int(np.abs(cur[0, 0].astype(int) - prv[0, 0]).sum()) if cur is flat else np.zeros_like(sad4))


def test_ties_resolve_by_the_stated_order():
    """a pattern of period 2 along x is, half a pixel to either side, the flat mean: against a flat frame of that mean the candidates (ey, -2) and
    (ey, +2) all have SAD4 = 0, so |v|_1 decides for ey = 0 and then the smaller dx4 for (0, -2); along y the same gives (-2, 0), which also beats
    (0, -2) on a checkerboard.  At Q = 4 the same candidates exist and win in the same order"""
    h, w = 24, 24
    y, x = np.mgrid[0:h, 0:w]
    cur = np.full((h, w, 3), 100, np.uint8)
    zero = np.zeros((3, 3, 2), np.int16)
    for pattern, want in ((x % 2, (0, -2)), (y % 2, (-2, 0)), ((x + y) % 2, (-2, 0))):
        prv = np.repeat((pattern * 200)[:, :, None], 3, axis=2).astype(np.uint8)
        for Q in ref.SUBPELS:
            for bias in (0, 4):
                vec4, sad4 = ref.refine_one(cur, prv, zero, 8, Q, bias)
                assert tuple(vec4[1, 1]) == want and sad4[1, 1] == 0, (want, Q, bias, vec4[1, 1])      # the block that no clamped border reaches
    # a vector out of the search's range is read clamped to +-2048, and the result fits int16
    far = np.full((3, 3, 2), 32767, np.int16)
    vec4, _ = ref.refine_one(cur, np.zeros_like(cur), far, 8, 4, 0)
    assert (vec4 == 4 * 2048 - 3).all()                          # all candidates tie: the shortest, then the smallest


# ---- the compensated recursion ---------------------------------------------------------------------------------------------------------------------
def _clip(n=5, H=23, W=31, seed=2):
    rs = np.random.RandomState(seed)
    G = rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)
    G[2] = G[1]
    return G, rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("down", [1, 2])
def test_mc_subpel_1_is_the_whole_pixel_stabiliser(down):
    f = ref.subshift(23, 31, 4, 4, 3, gain=1.0)
    Y = np.random.RandomState(3).randint(0, 256, f.shape, dtype=np.uint8)
    a = motion_ref.Stabiliser(down=down, mc_range=3, mc_block=8, mc_bias=4)
    b = ref.Stabiliser(down=down, mc_range=3, mc_block=8, mc_bias=4, mc_subpel=1)
    c = ref.Stabiliser(down=down, mc_range=3, mc_block=8, mc_bias=4, mc_subpel=4)
    differs = False
    for k in range(len(f)):
        want, got, fine = a.step(f[k], Y[k]), b.step(f[k], Y[k]), c.step(f[k], Y[k])
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4])) and np.array_equal(a.state, b.state), k
        assert (want[4] is None and got[4] is None) or np.array_equal(want[4], got[4])
        differs |= not np.array_equal(fine[0], want[0])
    assert differs or down > 1                                   # and at the frames' own resolution, where they move by quarters, the refined run is another run


def test_identical_hazy_frames_equal_the_whole_pixel_and_the_uncompensated_run():
    """SAD4(0) = 0 wins every tie, so the refined field is zero and the warp a copy"""
    G, Y = _clip()
    G[:] = G[0]
    want, _ = motion_ref.stabilise(G, Y)
    assert not np.array_equal(want, Y)
    for Q in (1, 2, 4):
        got, _ = ref.stabilise(G, Y, mc_range=4, mc_block=8, mc_bias=0, mc_subpel=Q)
        assert np.array_equal(got, want), Q


def test_the_restatement_does_not_depend_on_batching():
    """the device refines a batch in one launch; the restatement's batched refinement is frame by frame the one-frame refinement"""
    f = ref.subshift(20, 27, 4, 4, 3)
    vec, _ = motion_ref.search(f[1:], f[0], 8, 3, 4)
    vec4, sad4 = ref.refine(f[1:], f[0], vec, 8, 4, 4)
    for k in range(4):
        v1, s1 = ref.refine(f[k + 1:k + 2], f[k], vec[k:k + 1], 8, 4, 4)
        assert np.array_equal(v1[0], vec4[k]) and np.array_equal(s1[0], sad4[k])
    assert ref.fractional_share(vec4) >= 0.5


# ---- the experiment behind the flag -----------------------------------------------------------------------------------------------------------------
# motion_ref.PAN_SCENE's scene, frames and seed and PAN_JITTER at full resolution, stabilised at 1 / down of it; block 16, bias 4, range 4.
# (flicker along the true motion at full resolution in levels, PSNR against the clean frames from frame 4 on in dB) of: the network's frames,
# --temporal alone, --temporal_mc 4, refined to 1/2, refined to 1/4
EXPERIMENT = {
    "half": ((8.230, 31.673), (8.180, 31.713), (5.365, 34.050), (3.034, 36.835), (3.034, 36.835)),           # 192 x 256, (1, 3) per frame, down 2: (0.5, 1.5) working pixels
    "half_hard": ((7.870, 30.576), (6.987, 31.133), (5.448, 32.870), (4.440, 34.408), (4.441, 34.405)),      # the same over 40 % sky, with sensor noise of 2 levels
    "quarter": ((8.225, 31.678), (8.225, 31.678), (4.071, 35.422), (3.965, 35.647), (2.806, 37.170)),        # 384 x 512, (3, 5) per frame, down 4: (0.75, 1.25)
    "whole": ((8.165, 31.735), (8.165, 31.735), (1.369, 36.172), (1.369, 36.172), (1.369, 36.172)),          # 192 x 256, (2, 6) per frame, down 2: (1, 3)
}
HALF_BAR = 0.75              # flicker at Q = 2 against Q = 1 on "half" (measured 0.566)
QUARTER_BAR = 0.80           # flicker at Q = 4 against Q = 1 on "quarter" (measured 0.689); the margins cover a reseeded scene, not a kernel


@functools.lru_cache(maxsize=None)
def _scores(name):
    G, Y, J, origin = ref.clip(name)
    assert motion_ref.flicker_along_motion(J, origin) == 0
    rows = [ref.clip_scores(name, Y)] + [ref.clip_scores(name, ref.clip_run(name, Q)) for Q in (0, 1, 2, 4)]
    print("%s: %s" % (name, " | ".join("%.3f / %.3f dB" % r for r in rows)))
    return rows


@pytest.mark.parametrize("name", list(EXPERIMENT))
def test_the_experiment_is_pinned(name):
    """a pan that is a fraction of a working pixel per frame.  Whole-pixel compensation leaves every block misaligned by up to
    half a pixel and the motion test switches the recursion off on the edges; refinement recovers most of it.  The measured figures are pinned;
    the PSNR does not fall with refinement on any clip"""
    rows = _scores(name)
    assert np.allclose(rows, EXPERIMENT[name], atol=1e-3), rows
    assert rows[3][0] <= rows[2][0] and rows[4][0] <= rows[2][0]
    assert rows[3][1] >= rows[2][1] and rows[4][1] >= rows[2][1]


def test_refinement_recovers_the_fractional_pans():
    half, quarter = _scores("half"), _scores("quarter")
    assert half[3][0] <= HALF_BAR * half[2][0]
    assert quarter[4][0] <= QUARTER_BAR * quarter[2][0]
    for name in EXPERIMENT:
        rows = _scores(name)
        assert rows[3][1] >= rows[2][1] and rows[4][1] >= rows[2][1], name          # PSNR does not fall on any clip


def test_a_whole_pixel_pan_is_untouched_by_refinement():
    """where the motion is whole the refined field is 4 x the whole-pixel field and the run is the whole-pixel run, bit for bit"""
    want = ref.clip_run("whole", 1)
    for Q in ref.SUBPELS:
        assert np.array_equal(ref.clip_run("whole", Q), want), Q
    assert not np.array_equal(want, ref.clip_run("whole", 0))


# ---- the --temporal_mc_subpel option at parsing -------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    return VideoOptions().parse(["--in", "clip.y4m", "--out", str(tmp_path / "out.y4m"), "--name", "video", "--gpu_ids", "-1",
                                 "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_temporal_mc_subpel_flag_and_refusals(tmp_path, capsys):
    recorded = lambda: open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
    opt = _parse(tmp_path, "--temporal", "--temporal_mc", "4")
    plain_text, plain_rec = capsys.readouterr().out, recorded()
    assert "\ntemporal_mc_subpel" not in plain_text and "\ntemporal_mc_subpel" not in plain_rec and "\ntemporal_mc: 4" in plain_text
    assert not getattr(opt, "temporal_mc_subpel", None)
    opt = _parse(tmp_path, "--temporal", "--temporal_mc", "4", "--temporal_mc_subpel", "1")          # the default, given: the run without the flag
    assert opt.temporal_mc_subpel == 1 and capsys.readouterr().out == plain_text and recorded() == plain_rec
    for args in ((), ("--temporal",)):
        _parse(tmp_path, *args)
        assert "\ntemporal_mc" not in capsys.readouterr().out and "\ntemporal_mc" not in recorded()
    for q in (2, 4):
        opt = _parse(tmp_path, "--temporal", "--temporal_mc", "8", "--temporal_mc_subpel", str(q), "--fit", "--eval_noref", "--eval_flicker")
        assert (opt.temporal_mc, opt.temporal_mc_subpel) == (8, q)
        assert "temporal_mc_subpel: %d" % q in capsys.readouterr().out and "temporal_mc_subpel: %d" % q in recorded()
    for args in (("--temporal_mc_subpel", "2"), ("--temporal", "--temporal_mc_subpel", "2"), ("--temporal", "--temporal_mc", "0", "--temporal_mc_subpel", "4"),
                 ("--temporal", "--temporal_mc_subpel", "1")):
        with pytest.raises(ValueError) as e:                     # it needs --temporal and --temporal_mc > 0
            _parse(tmp_path, *args)
        assert "--temporal_mc_subpel" in str(e.value) and "only applies with --temporal" in str(e.value), str(e.value)
    capsys.readouterr()
    for v in ("0", "3", "8", "-2", "2.5", "x"):
        with pytest.raises(SystemExit) as e:                     # any other value: argparse leaves with 2 and names the flag
            _parse(tmp_path, "--temporal", "--temporal_mc", "4", "--temporal_mc_subpel", v)
        assert e.value.code == 2 and "--temporal_mc_subpel" in capsys.readouterr().err


def test_the_help_text_says_where_the_evidence_comes_from():
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    o = VideoOptions()
    o.initialize()
    text = " ".join(o.parser.format_help().split())
    tail = text.split("--temporal_mc_subpel {1,2,4}")[-1].split("--eval_flicker")[0]
    assert "synthetic panning experiment" in tail and "not footage" in tail and "DESIGN section 25" in tail


def test_check_mc_subpel():
    from cfen_vit_dehazing_amd import temporal
    assert temporal.MC_SUBPEL == (1, 2, 4) and temporal.MC_DEFAULTS == {"range": 0, "block": 16, "bias": 4}
    assert [temporal.check_mc_subpel(q) for q in (1, 2, 4, np.int64(4), 2.0)] == [1, 2, 4, 4, 2]
    assert temporal.check_mc_subpel(1, 0) == 1 and temporal.check_mc_subpel(4, 8) == 4
    for bad in (0, 3, 8, -2, 2.5, None, "2"):
        with pytest.raises(ValueError, match="Stabiliser: mc_subpel must be 1, 2 or 4"):
            temporal.Stabiliser(mc_range=4, mc_subpel=bad)
    for q in (2, 4):
        with pytest.raises(ValueError, match="mc_subpel = %d .* needs mc_range > 0" % q):
            temporal.Stabiliser(mc_subpel=q)
    with pytest.raises(TypeError):
        temporal.Stabiliser(2, 1e-4, 0.8, 8.0, "auto", 4, 16, 4, 2)                       # keyword-only, as the other mc arguments
    st = temporal.Stabiliser(mc_range=4, mc_subpel=2)
    assert (st.mc_range, st.mc_block, st.mc_bias, st.mc_subpel) == (4, 16, 4, 2)
    assert temporal.Stabiliser().mc_subpel == 1 and temporal.Stabiliser(mc_range=4).mc_subpel == 1


# ---- the new header's ledger ------------------------------------------------------------------------------------------------------------------------
FNS = {"cfen_motion_refine_u8": 12, "cfen_motion_warp_subpel": 9}


def test_subpel_header_is_exported_bound_and_apart_from_the_older_tables():
    cabi_ledger.check_header_bound("cfen_subpel.h", FNS)
    cabi_ledger.check_guard_band_test_calls("test_hip_subpel.py", "test_guard_bands_subpel", FNS)
    _lib = cabi_ledger.library()
    assert len(_lib.SIGNATURES) == 68 and _lib.load().cfen_abi_version() == 1
    assert sorted(_lib.HEADERS["cfen_motion.h"]) == ["cfen_motion_search_u8", "cfen_motion_warp"]


def test_the_definition_stands_in_the_header():
    text = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "cfen_subpel.h")).read()).split())
    for phrase in ("y0 = y4 >> 2 (arithmetic shift, i.e. the floor) and fy = y4 & 3",
                   "S(y4, x4, c) = ((4-fy)(4-fx)*p00 + (4-fy)*fx*p01 + fy*(4-fx)*p10 + fy*fx*p11 + 8) >> 4",
                   "each coordinate is clamped to the frame on its own", "read clamped to +-2048",
                   "v4 = 4*v0 + (ey, ex)*(4/Q) for ey, ex in -(Q-1) .. Q-1", "9 candidates at Q = 2 and 49 at Q = 4",
                   "SAD4(v4) = sum_{p in block} sum_c |I_t(p, c) - S(4p + v4, c)|", "cost4(v4) = 64*SAD4 + bias*(|dy4| + |dx4|)*3*n_b",
                   "lexicographically smallest (cost4, |dy4| + |dx4|, dy4, dx4)", "prev_out(p, c) = S(4p + v4_b, c)",
                   "t0 = s00 + fx*(s01 - s00)", "t1 = s10 + fx*(s11 - s10)", "state_out = t0 + fy*(t1 - t0)",
                   "A multiply and the add after it may fuse", "multiples of 4 makes the warp equal to cfen_motion_warp with vec4/4",
                   "SAD4(0) = 0, which wins every tie", "does not depend on how frames are grouped into batches", "block in {8, 16, 32}; subpel in {2, 4}"):
        assert phrase in text, phrase


# ---- the C entry points refuse bad arguments before any launch --------------------------------------------------------------------------------------
def test_subpel_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    g, p, v, v4, s, st, po, so, z = (ctypes.c_void_p(k << 20) for k in (1, 2, 3, 4, 5, 6, 7, 8, 0))      # never dereferenced
    refused, off = functools.partial(cabi_ledger.refused, lib), cabi_ledger.off

    def refine(gg=g, pp=p, vv=v, B=1, h=20, w=20, block=8, subpel=2, bias=4, vv4=v4, ss=s):
        return (gg, pp, vv, B, h, w, block, subpel, bias, vv4, ss, z)

    for name in ("gg", "pp", "vv", "vv4", "ss"):
        refused("motion_refine_u8", b"null pointer", *refine(**{name: z}))
    refused("motion_refine_u8", b"B = 0", *refine(B=0))
    refused("motion_refine_u8", b"B = 65537", *refine(B=65537))
    refused("motion_refine_u8", b"h = 0", *refine(h=0))
    refused("motion_refine_u8", b"w = 16385", *refine(w=16385))
    for block in (0, 4, 12, 64, -8):
        refused("motion_refine_u8", b"block = %d" % block, *refine(block=block))
    for q in (0, 1, 3, 8, -2):
        refused("motion_refine_u8", b"subpel = %d" % q, *refine(subpel=q))
    refused("motion_refine_u8", b"bias = -1", *refine(bias=-1))
    refused("motion_refine_u8", b"bias = 256", *refine(bias=256))
    for bad in ({"vv": off(v, 2)}, {"vv4": off(v4, 1)}, {"ss": off(s, 2)}):
        refused("motion_refine_u8", b"4-byte aligned", *refine(**bad))
    # B = 2 frames of 20 x 20: guide 2400 bytes, prev_guide 1200, vec, vec4 and sad4 2 * 9 * 4 = 72
    for bad in ({"pp": g}, {"pp": off(g, 2399)}, {"pp": off(g, -1199)}, {"vv4": v}, {"vv4": off(v, 68)}, {"ss": off(v, -68)}, {"ss": v4}, {"vv": g},
                {"ss": off(p, 1196)}):
        refused("motion_refine_u8", b"must not overlap", *refine(B=2, **bad))

    for bad in ((z, p, st, po, so), (v4, z, st, po, so), (v4, p, z, po, so), (v4, p, st, z, so), (v4, p, st, po, z)):
        refused("motion_warp_subpel", b"null pointer", bad[0], bad[1], bad[2], 20, 20, 8, bad[3], bad[4], z)
    refused("motion_warp_subpel", b"h = 0", v4, p, st, 0, 20, 8, po, so, z)
    refused("motion_warp_subpel", b"w = 16385", v4, p, st, 20, 16385, 8, po, so, z)
    for block in (0, 12, 64):
        refused("motion_warp_subpel", b"block = %d" % block, v4, p, st, 20, 20, block, po, so, z)
    refused("motion_warp_subpel", b"4-byte aligned", off(v4, 2), p, st, 20, 20, 8, po, so, z)
    for bad in ((off(st, 8), so), (st, off(so, 4))):
        refused("motion_warp_subpel", b"16-byte aligned", v4, p, bad[0], 20, 20, 8, po, bad[1], z)
    # 20 x 20: vec4 36 bytes, prev_guide and prev_out 1200, state and state_out 9600
    for bad in ((v4, p, st, p, so), (v4, p, st, po, st), (v4, p, st, off(p, 1199), so), (v4, p, st, po, off(st, 9584)), (v4, p, st, off(v4, 35), so),
                (v4, p, st, po, off(po, 1184)), (v4, off(st, 9599), st, po, so)):
        refused("motion_warp_subpel", b"must not overlap", bad[0], bad[1], bad[2], 20, 20, 8, bad[3], bad[4], z)


def test_no_ashr_pk_u8_in_the_build():
    """the integer-bilinear bytes are shifted, never clamped: the instruction DESIGN section 17 found wrong must not appear"""
    from cfen_vit_dehazing_amd import build
    cabi_ledger.library()
    n = build.check_no_ashr_pk_u8()
    assert n in (0, None)
