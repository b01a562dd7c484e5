"""Motion compensation on the device (cfen_motion_search_u8, cfen_motion_warp; ops.motion_search_u8, ops.motion_warp,
temporal.Stabiliser(mc_range=...), dehaze_video.py --temporal_mc).  The search and the warp are integer and gathers: they are held to the
restatement tests/motion_ref.py bit for bit.  The compensated recursion carries the tolerance TAU_T of tests/test_temporal_host.py and the
byte rule of tests/test_hip_temporal.py, unchanged; the determinism, composition and end-to-end tests have no tolerance."""
import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, temporal
import guarded
import motion_ref as ref
import temporal_ref
import yuv_ref
from test_hip_temporal import CLIPS, _at_offset, assert_bytes
from test_temporal_host import TAU_T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIAS = temporal.MC_DEFAULTS["bias"]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared reference arrays are read-only


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


# ---- search ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", ref.RANGES)
@pytest.mark.parametrize("block", ref.BLOCKS)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_search_bitwise(h, w, block, R):
    """vec and sad of every kind of content and both biases: three frames in one call, the first frame alone, and the three frames behind a
    prev_guide that is a copy of the first (frame 0 then returns zeros with sad 0)"""
    moved = 0
    for kind in ref.KINDS:
        for bias in (0, BIAS):
            guide, prev, vec, sad = ref.search_case(kind, h, w, block, R, bias, 3)
            tg, tp = dev(guide), dev(prev)
            v3, s3 = ops.motion_search_u8(tg, tp, block, R, bias)
            assert v3.shape == vec.shape and v3.dtype == torch.int16 and s3.shape == sad.shape and s3.dtype == torch.int32
            assert same(v3, vec) and same(s3, sad), (kind, bias)
            v1, s1 = ops.motion_search_u8(tg[:1], tp, block, R, bias)
            assert same(v1, vec[:1]) and same(s1, sad[:1]), (kind, bias)
            vs, ss = ops.motion_search_u8(tg, tg[0].clone(), block, R, bias)
            assert not vs[0].any() and not ss[0].any() and same(vs[1:], vec[1:]) and same(ss[1:], sad[1:]), (kind, bias)
            moved += int(np.any(vec))
            if kind == "flat":
                assert not vec.any()                             # all ties: the bias and the shorter vector decide for (0, 0)
    assert moved == (0 if (h, w) == (1, 1) else 6)               # every kind but the flat one moves, except in the frame of one pixel


def test_the_cases_reach_every_branch():
    """what the contents are for, shown on the restatement: non-zero vectors, vectors at +-range, partial blocks, winners whose window was clamped"""
    guide, prev, vec, sad = ref.search_case("shift", 40, 50, 8, 3, BIAS, 3)
    assert (np.abs(vec).max(axis=(0, 1, 2)) > 0).all() and sad.max() > 0
    guide, prev, vec, sad = ref.search_case("border", 40, 50, 16, 16, 0, 3)
    bh, bw, _ = ref.grid(40, 50, 16)
    x0, y0 = np.arange(bw) * 16, np.arange(bh) * 16
    x1, y1 = np.minimum(x0 + 16, 50) - 1, np.minimum(y0 + 16, 40) - 1
    crossing = (x1[None, None, :] + vec[..., 1] > 49) | (x0[None, None, :] + vec[..., 1] < 0) | (y1[None, :, None] + vec[..., 0] > 39) | \
        (y0[None, :, None] + vec[..., 0] < 0)
    assert crossing.sum() >= 8                                   # winners whose window reaches across the clamped border
    guide, prev, vec, sad = ref.search_case("random", 17, 33, 16, 16, 0, 3)
    assert np.abs(vec).max() > 8 and vec.shape == (3, 2, 3, 2)


# ---- warp -----------------------------------------------------------------------------------------------------------------------------------------
def _warp_inputs(h, w, block, R, seed):
    rs = np.random.RandomState(seed)
    bh, bw, _ = ref.grid(h, w, block)
    vec = rs.choice([-R, R, 0, rs.randint(-R, R + 1)], size=(bh, bw, 2)).astype(np.int16)
    return vec, rs.randint(0, 256, (h, w, 3), dtype=np.uint8), rs.normal(0, 100, (h, w, 6)).astype(np.float32)


@pytest.mark.parametrize("block", ref.BLOCKS)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_warp_bitwise(h, w, block):
    for R in ref.RANGES:
        vec, prev, state = _warp_inputs(h, w, block, R, h + w + block + R)
        want_p, want_s = ref.warp(vec, prev, state, block)
        got_p, got_s = ops.motion_warp(dev(vec), dev(prev), dev(state), block)
        assert got_p.dtype == torch.uint8 and got_s.dtype == torch.float32 and same(got_p, want_p) and same(got_s, want_s), R
    zero_p, zero_s = ops.motion_warp(dev(np.zeros_like(vec)), dev(prev), dev(state), block)
    assert same(zero_p, prev) and same(zero_s, state)            # a zero field is a copy


# ---- unaligned buffers, a side stream, batching -----------------------------------------------------------------------------------------------------
def test_byte_offsets_and_a_side_stream():
    """guide, prev_guide and prev_out each 1 .. 3 bytes past a 16-byte boundary, and both calls on a side stream: the same results"""
    h, w, block, R = 17, 33, 8, 3
    guide, prev, vec, sad = ref.search_case("shift", h, w, block, R, BIAS, 3)
    wvec, wprev, wstate = _warp_inputs(h, w, block, R, 9)
    want_p, want_s = ref.warp(wvec, wprev, wstate, block)
    tv, ts = dev(wvec), dev(wstate)
    for k in (1, 2, 3):
        for ks in ((k, 0), (0, k), (k, (k + 1) % 4)):
            v, s = ops.motion_search_u8(_at_offset(guide, ks[0]), _at_offset(prev, ks[1]), block, R, BIAS)
            assert same(v, vec) and same(s, sad), ks
            out = (_at_offset(np.zeros((h, w, 3), np.uint8), ks[1]), torch.empty(h, w, 6, device=DEV))
            p, st = ops.motion_warp(tv, _at_offset(wprev, ks[0]), ts, block, out=out)
            assert p.data_ptr() == out[0].data_ptr() and same(p, want_p) and same(st, want_s), ks
    tg, tp, twp = dev(guide), dev(prev), dev(wprev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v, s = ops.motion_search_u8(tg, tp, block, R, BIAS)
        p, st = ops.motion_warp(tv, twp, ts, block)
    side.synchronize()
    assert same(v, vec) and same(s, sad) and same(p, want_p) and same(st, want_s)


def test_one_call_on_four_frames_is_four_calls_of_one():
    f = ref.frames("shift", 40, 50, 4, 6)
    tf = dev(f)
    vec, sad = ops.motion_search_u8(tf[1:], tf[0], 16, 3, BIAS)
    for k in range(4):
        v1, s1 = ops.motion_search_u8(tf[k + 1:k + 2], tf[k], 16, 3, BIAS)
        assert torch.equal(v1[0], vec[k]) and torch.equal(s1[0], sad[k]), k
    for _ in range(2):                                           # repeated calls
        v, s = ops.motion_search_u8(tf[1:], tf[0], 16, 3, BIAS)
        assert torch.equal(v, vec) and torch.equal(s, sad)
    assert bool(vec.any())


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_motion():
    """every input between 0xff bands, every output between random bands, prefilled 0xff, zeros and random bytes, for both entry points: no band
    changes, and the payload is the restatement's whatever it held before"""
    lib = _lib.load()
    for (h, w), block, R in (((17, 33), 8, 3), ((40, 50), 32, 16), ((5, 7), 16, 1)):
        guide, prev, vec, sad = ref.search_case("shift", h, w, block, R, BIAS, 3)
        wvec, wprev, wstate = _warp_inputs(h, w, block, R, 3)
        want_p, want_s = ref.warp(wvec, wprev, wstate, block)
        tg, tp = guarded.guarded_copy(dev(guide)), guarded.guarded_copy(dev(prev))
        tv, twp, tws = guarded.guarded_copy(dev(wvec)), guarded.guarded_copy(dev(wprev)), guarded.guarded_copy(dev(wstate))
        ov = guarded.guarded_empty(vec.shape, torch.int16, DEV)
        os_ = guarded.guarded_empty(sad.shape, torch.int32, DEV)
        op = guarded.guarded_empty((h, w, 3), torch.uint8, DEV)
        ost = guarded.guarded_empty((h, w, 6), torch.float32, DEV)
        for fill in guarded.FILLS:
            for t in (ov, os_, op, ost):
                guarded.refill(t, fill)
            _lib.check(lib.cfen_motion_search_u8(_lib.ptr(tg), _lib.ptr(tp), 3, h, w, block, R, BIAS, _lib.ptr(ov), _lib.ptr(os_), _lib.current_stream()),
                       "motion_search_u8")
            _lib.check(lib.cfen_motion_warp(_lib.ptr(tv), _lib.ptr(twp), _lib.ptr(tws), h, w, block, _lib.ptr(op), _lib.ptr(ost), _lib.current_stream()),
                       "motion_warp")
            torch.cuda.synchronize()
            guarded.check_bands(tg, tp, ov, os_, tv, twp, tws, op, ost)
            assert same(ov, vec) and same(os_, sad) and same(op, want_p) and same(ost, want_s), (h, w, fill)


def test_argument_errors_launch_nothing():
    h, w = 20, 20
    f = dev(ref.frames("random", h, w, 2, 1))
    vec = torch.full((2, 3, 3, 2), 7, dtype=torch.int16, device=DEV)
    sad = torch.full((2, 3, 3), 7, dtype=torch.int32, device=DEV)
    for bad in ({"block": 12}, {"block": 8.5}, {"range": 0}, {"range": 17}, {"range": 2.5}, {"bias": -1}, {"bias": 256}):
        with pytest.raises(ValueError, match="motion_search_u8: (block|range|bias)"):
            ops.motion_search_u8(f[1:], f[0], **dict({"block": 8, "range": 2, "bias": 4}, **bad), out=(vec, sad))
    with pytest.raises(ValueError, match="needs prev_guide"):
        ops.motion_search_u8(f[1:], f[0, :10], 8, 2, 4)
    with pytest.raises(ValueError, match="out must be"):
        ops.motion_search_u8(f[1:], f[0], 8, 2, 4, out=(vec[:1], sad))
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_search_u8(f[1:], f[1], 8, 2, 4, out=(vec, sad))
    state = torch.full((h, w, 6), 7.0, device=DEV)
    out = (torch.full((h, w, 3), 9, dtype=torch.uint8, device=DEV), torch.full((h, w, 6), 9.0, device=DEV))
    with pytest.raises(ValueError, match="motion_warp needs vec"):
        ops.motion_warp(vec[0, :2], f[0], state, 8, out=out)
    with pytest.raises(ValueError, match="motion_warp needs state"):
        ops.motion_warp(vec[0], f[0], state[:4], 8, out=out)
    with pytest.raises(ValueError, match="motion_warp: block"):
        ops.motion_warp(vec[0], f[0], state, 4, out=out)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_warp(vec[0], f[0], state, 8, out=(f[0], out[1]))
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_warp(vec[0], f[0], state, 8, out=(out[0], state))
    torch.cuda.synchronize()
    assert bool((vec == 7).all()) and bool((sad == 7).all()) and bool((out[0] == 9).all()) and bool((out[1] == 9.0).all()) and bool((state == 7.0).all())


# ---- the compensated recursion ---------------------------------------------------------------------------------------------------------------------
def _compose(tG, tY, radius=2, eps=1e-4, strength=0.8, motion=8.0, down=1, mc_range=4, mc_block=16, mc_bias=BIAS):
    """the compensated Stabiliser written out with the operators, frame by frame: (frames, state, every delta)"""
    n, H, W, _ = tG.shape
    S, h, w = temporal.working_size(H, W, down)
    I, P = (tG, tY) if S == 1 else (ops.resample_u8(tG, (h, w), filter="box"), ops.resample_u8(tY, (h, w), filter="box"))
    coef = ops.guided_coef_u8(I, P, radius, eps)
    state = torch.empty(h, w, 6, device=DEV)
    deltas = [ops.temporal_blend(I[:1], None, coef[:1], state, radius, motion, strength, False)]
    for k in range(1, n):
        vec, _ = ops.motion_search_u8(I[k:k + 1], I[k - 1], mc_block, mc_range, mc_bias)
        warped, state = ops.motion_warp(vec[0], I[k - 1], state, mc_block)
        deltas.append(ops.temporal_blend(I[k:k + 1], warped, coef[k:k + 1].clone(), state, radius, motion, strength, True))          # (a 16-byte aligned copy)
    delta = torch.cat(deltas)
    return ops.temporal_apply_u8(delta, tG, tY), state, delta


def _pan(n, H, W, seed, step=(1, 3)):
    """hazy and dehazed frames of a window that moves over a random blocky-and-noisy picture, and flickering outputs"""
    rs = np.random.RandomState(seed)
    big = np.repeat(np.repeat(rs.randint(30, 226, ((H + 88) // 4 + 1, (W + 88) // 4 + 1, 3)), 4, axis=0), 4, axis=1)[:H + 88, :W + 88]
    big = big + rs.randint(-12, 13, big.shape)
    G = np.stack([np.clip(big[step[0] * k:step[0] * k + H, step[1] * k:step[1] * k + W], 0, 255) for k in range(n)]).astype(np.uint8)
    Y = np.clip(0.9 * G + rs.normal(0, 6, (n, 1, 1, 3)) + rs.randint(-2, 3, G.shape) - 20, 0, 255).astype(np.uint8)
    return G, Y


@pytest.mark.parametrize("H,W,down,block", [(40, 64, 1, 16), (75, 101, 2, 8), (45, 71, 1, 32)])          # the last: odd h w, frames of a batch 8 bytes off
def test_stabiliser_is_the_composition_of_its_operators_and_does_not_depend_on_batching(H, W, down, block):
    G, Y = _pan(5, H, W, H, step=(down, 3 * down))              # (1, 3) pixels per frame at the working resolution
    tG, tY = dev(G), dev(Y)
    want, state, _ = _compose(tG, tY, down=down, mc_block=block, mc_range=4)
    plain = temporal.Stabiliser(down=down).step(tG, tY)
    assert torch.equal(want[0], tY[0]) and not torch.equal(want, plain)                  # the field is not zero: compensation changes the bytes
    for sizes in ((5,), (1, 1, 1, 1, 1), (2, 2, 1), (1, 4), (3, 2)):                      # batches of 1, 2 and 5, and mixtures
        st = temporal.Stabiliser(down=down, mc_range=4, mc_block=block)
        parts, lo = [], 0
        for m in sizes:
            parts.append(st.step(tG[lo:lo + m], tY[lo:lo + m]))
            lo += m
        assert torch.equal(torch.cat(parts), want) and torch.equal(st._state, state), sizes
    st.reset()                                                   # reset() starts a new stream and clears the extra buffers; out= is used
    assert st._state2 is None and st._warped is None and st._vec is None
    out = torch.empty_like(tY)
    assert st.step(tG, tY, out=out).data_ptr() == out.data_ptr() and torch.equal(out, want)


def test_the_compensated_recursion_against_float64():
    """given coefficients (temporal_ref.coefficients, as test_blend_against_float64 is given them), four frames of a moving texture: the device's
    search -> warp -> blend (B = 1) chain against the float64 restatement of the same chain; Delta and S within TAU_T, the bytes by assert_bytes"""
    h, w, block, R, r = 40, 50, 16, 3, 2
    f = ref.frames("shift", h, w, 3, 12)
    coef = temporal_ref.coefficients(4, h, w, 12) * np.float32(0.1)
    Y = np.random.RandomState(12).randint(0, 256, f.shape, dtype=np.uint8)
    tf, tc = dev(f), dev(coef)
    state = torch.full((h, w, 6), float("nan"), device=DEV)
    deltas = [ops.temporal_blend(tf[:1], None, tc[:1], state, r, temporal_ref.MOTION, temporal_ref.STRENGTH, False)]
    d64, s64, _, _ = temporal_ref.blend(f[:1], None, coef[:1], r, temporal_ref.MOTION, temporal_ref.STRENGTH, None)
    want = [d64[0]]
    kept = 0
    for k in range(1, 4):
        vec, _ = ops.motion_search_u8(tf[k:k + 1], tf[k - 1], block, R, BIAS)
        warped, state = ops.motion_warp(vec[0], tf[k - 1], state, block)
        deltas.append(ops.temporal_blend(tf[k:k + 1], warped, tc[k:k + 1], state, r, temporal_ref.MOTION, temporal_ref.STRENGTH, True))
        v64 = ref.search_one(f[k], f[k - 1], block, R, BIAS)[0]
        assert same(vec[0], v64) and v64.any()
        p64, sw64 = ref.warp(v64, f[k - 1], s64, block)
        d64, s64, keep, _ = temporal_ref.blend(f[k:k + 1], p64, coef[k:k + 1], r, temporal_ref.MOTION, temporal_ref.STRENGTH, sw64)
        want.append(d64[0])
        kept += int((keep > 0).sum())
    assert kept                                                  # the recursion was on somewhere: the warp brought matching pixels under the window
    delta = torch.cat(deltas)
    ed = np.abs(delta.cpu().numpy().astype(np.float64) - np.stack(want)).max()
    es = np.abs(state.cpu().numpy().astype(np.float64) - s64).max()
    print("compensated chain: max |dDelta| %.3e, |dS| %.3e (TAU_T %.3e), keep > 0 on %d pixel-frames" % (ed, es, TAU_T, kept))
    assert ed <= TAU_T and es <= TAU_T
    got = ops.temporal_apply_u8(delta, tf, dev(Y)).cpu().numpy()
    assert_bytes(got, np.stack([temporal_ref.apply_v(want[k], f[k], Y[k]) for k in range(4)]), "compensated chain")


def test_identical_hazy_frames_equal_the_uncompensated_run():
    """SAD(0) = 0 wins every tie: the field is zero, the warp a copy, and mc_range = 4 is mc_range = 0 bit for bit"""
    G, Y = _pan(4, 45, 70, 3)
    tG, tY = dev(G[:1]).repeat(4, 1, 1, 1), dev(Y)
    for down in (1, 2):
        want = temporal.Stabiliser(down=down).step(tG, tY)
        assert not torch.equal(want, tY)
        for block in ref.BLOCKS:
            st = temporal.Stabiliser(down=down, mc_range=4, mc_block=block, mc_bias=0)
            assert torch.equal(st.step(tG, tY), want) and not bool(st._vec[:3].any()) and not bool(st._sad[:3].any())          # (the first frame is not searched)


def test_the_panning_clip_flickers_less_on_the_device():
    """the clip of DESIGN section 20 at the defaults: the device's frames against the float64 restatement's by the bar of
    test_hip_temporal.test_stabiliser_is_the_composition_of_its_operators (the coefficients of step 2 carry the tolerance of
    tests/test_hip_guided.py: a byte differs by at most 1, on fewer than one byte in a hundred), so the flicker along the motion, a mean of
    differences of neighbouring frames' bytes, agrees within twice that share; and it is below the uncompensated device run's"""
    block = temporal.MC_DEFAULTS["block"]
    G, Y, J, origin, ref_alone, ref_mc = ref.panning_case(block, BIAS)
    tG, tY = dev(G), dev(Y)
    got = temporal.Stabiliser(mc_range=ref.PAN_RANGE).step(tG, tY).cpu().numpy()
    alone = temporal.Stabiliser().step(tG, tY).cpu().numpy()
    diff = np.abs(got.astype(np.int64) - ref_mc)
    share = (diff != 0).mean()
    fl = [ref.flicker_along_motion(x, origin) for x in (Y, alone, got, ref_mc)]
    print("flicker along the motion: network %.3f, device alone %.3f, device compensated %.3f, restatement %.3f; %d of %d bytes differ"
          % (fl[0], fl[1], fl[2], fl[3], (diff != 0).sum(), diff.size))
    assert diff.max() <= 1 and share < 0.01
    assert abs(fl[2] - fl[3]) <= 2 * share + 1e-12
    assert fl[2] < fl[1] and fl[2] < fl[0]


# ---- dehaze_video.py --temporal_mc -------------------------------------------------------------------------------------------------------------------
def _panned_stream(n, H, W, chroma, seed=23):
    """a y4m stream of a window moving (1, 3) pixels per frame over a blocky picture, and the frames' RGB by the restatement"""
    G, _ = _pan(n, H, W, seed)
    frames = [yuv_ref.rgb_to_yuv(g, chroma, "bt601", False) for g in G]
    header = yuv_ref.y4m_header(W, H, chroma)
    return yuv_ref.y4m_bytes(frames, W, H, chroma, header=header), header, [yuv_ref.yuv_to_rgb(f, H, W, chroma, "bt601", False) for f in frames]


@pytest.mark.parametrize("route", list(CLIPS))
def test_cli_temporal_mc(route, tmp_path):
    """dehaze_video.py --temporal --temporal_mc 4 in a child process: the stream is, bit for bit, library route -> Stabiliser(mc_range=4).step -> the
    restatement's RGB -> YCbCr; the same clip without the flag is the uncompensated Stabiliser's, as before"""
    import test_hip_video as vid
    n, H, W, chroma, flags = CLIPS[route]
    vid._setup(tmp_path)
    data, header, rgb = _panned_stream(n, H, W, chroma)
    (tmp_path / "in.y4m").write_bytes(data)
    net = vid._net()
    x = dev(np.stack(rgb))
    with torch.no_grad():
        outs = []
        for lo in range(0, n, 2):
            if route == "plain":
                net.output_u8 = True
                outs.append(net(x[lo:lo + 2])[2])
                net.output_u8 = False
            else:
                outs.append(net.forward_fit(x[lo:lo + 2])[2])
    y = torch.cat(outs).contiguous()
    st, plain = temporal.Stabiliser(mc_range=4), temporal.Stabiliser()
    stab = torch.cat([st.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
    alone = torch.cat([plain.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
    assert torch.equal(stab[0], y[0]) and not torch.equal(stab, alone)
    print("%s: compensation changes %.1f %% of the bytes of the uncompensated run" % (route, 100 * (stab != alone).float().mean().item()))

    def check(out_bytes, want):
        got_header, got = yuv_ref.y4m_frames(out_bytes, H, W, chroma)
        assert got_header == header and len(got) == n
        for k in range(n):
            assert np.array_equal(got[k], yuv_ref.rgb_to_yuv(want[k], chroma, "bt601", False)), (route, k)

    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "mc.y4m", flags + ["--batchSize", "2", "--temporal", "--temporal_mc", "4"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    text = r.stdout.decode()
    assert "temporal_mc: 4" in text and "temporal_mc_block: 16" in text and "video: motion compensation within +-4 pixels, blocks of 16 x 16" in text
    check((tmp_path / "mc.y4m").read_bytes(), stab.cpu().numpy())
    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "alone.y4m", flags + ["--batchSize", "2", "--temporal"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "temporal_mc" not in r.stdout.decode().replace(str(tmp_path), "") and "video: motion compensation" not in r.stdout.decode()
    check((tmp_path / "alone.y4m").read_bytes(), alone.cpu().numpy())
    if route == "plain":                                       # a refusal leaves with 2 and writes nothing
        r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "none.y4m", ["--temporal", "--temporal_mc", "17"])
        assert r.returncode == 2 and b"--temporal_mc" in r.stderr and not (tmp_path / "none.y4m").exists()
        r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "none.y4m", ["--temporal_mc", "4"])
        assert r.returncode == 2 and b"--temporal" in r.stderr and not (tmp_path / "none.y4m").exists()
