"""Sub-pixel motion compensation on the device (cfen_motion_refine_u8, cfen_motion_warp_subpel; ops.motion_refine_u8, ops.motion_warp_subpel,
temporal.Stabiliser(mc_subpel=...), dehaze_video.py --temporal_mc_subpel).  The refinement and the warped bytes are integer: they are held to the
restatement tests/subpel_ref.py bit for bit.  The warped state is a lerp of four fp32 taps in fp32: it is held to the float64 restatement
within 32 * 2^-24 * M, M the largest magnitude among the four taps -- a bound that is derived, not measured: the header's order has at most
about sixteen roundings, each of a value no larger than 2 M, while a wrong tap or weight misses by a quarter of a tap difference.  The
compensated recursion carries the tolerance TAU_T of tests/test_temporal_host.py and the byte rule of tests/test_hip_temporal.py, unchanged;
the composition, batching and end-to-end tests have no tolerance.  CFEN_WRITE_PARITY=1 writes the device's figures on the experiment's first
clip to profiles/subpel_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, temporal
import guarded
import motion_ref
import subpel_ref as ref
import temporal_ref
import yuv_ref
from test_hip_temporal import CLIPS, _at_offset, assert_bytes
from test_hip_video_deep import ckpt          # noqa: F401  (the module-scoped checkpoint fixture: one file, linked where one exists, removed with the module)
from test_temporal_host import TAU_T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BIAS = temporal.MC_DEFAULTS["bias"]
STATE_BOUND = 32 * 2.0 ** -24          # times the largest tap magnitude


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared reference arrays are read-only


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


# ---- refinement -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", ref.SUBPELS)
@pytest.mark.parametrize("block", ref.BLOCKS)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_refine_bitwise(h, w, block, Q):
    """vec4 and sad4 of every kind of content, both biases, the restatement's own whole-pixel field and a hand-made one at +-16 whose taps cross
    the clamped border: three frames in one call, the first frame alone, and the three frames behind a prev_guide that is a copy of the first"""
    fractional = 0
    for kind in ref.KINDS:
        for bias in ref.BIASES:
            for hand in (False, True):
                guide, prev, vec, vec4, sad4 = ref.refine_case(kind, h, w, block, Q, bias, 3, hand)
                tg, tp, tv = dev(guide), dev(prev), dev(vec)
                v3, s3 = ops.motion_refine_u8(tg, tp, tv, block, Q, bias)
                assert v3.shape == vec4.shape and v3.dtype == torch.int16 and s3.shape == sad4.shape and s3.dtype == torch.int32
                assert same(v3, vec4) and same(s3, sad4), (kind, bias, hand)
                v1, s1 = ops.motion_refine_u8(tg[:1], tp, tv[:1], block, Q, bias)
                assert same(v1, vec4[:1]) and same(s1, sad4[:1]), (kind, bias, hand)
                want_v, want_s = ref.refine(guide, guide[0], vec, block, Q, bias)
                vs, ss = ops.motion_refine_u8(tg, tg[0].clone(), tv, block, Q, bias)
                assert same(vs, want_v) and same(ss, want_s) and np.array_equal(want_v[1:], vec4[1:]), (kind, bias, hand)
                if not hand and not vec[0].any():
                    assert not want_v[0].any() and not want_s[0].any()            # an identical predecessor and a zero field: SAD4(0) = 0 wins
                fractional += int(kind == "subshift" and not hand and ref.fractional_share(vec4) >= 0.5)
                if kind == "flat" and not hand:
                    assert not vec4.any()
    assert fractional == (0 if (h, w) == (1, 1) else 2)          # the subshift fields are fractional at both biases, except in the frame of one pixel


def test_the_cases_reach_every_branch():
    """what the contents are for, shown on the restatement: fractional winners in every direction, partial blocks, winners whose taps were clamped"""
    _, _, vec, vec4, sad4 = ref.refine_case("subshift", 40, 50, 8, 4, BIAS, 3)
    frac = (vec4.astype(int) - 4 * vec).reshape(-1, 2)
    assert (frac != 0).any(axis=0).all() and (frac > 0).any() and (frac < 0).any() and sad4.max() > 0
    _, _, vec, vec4, _ = ref.refine_case("border", 40, 50, 16, 4, 0, 3, True)
    bh, bw, _ = ref.grid(40, 50, 16)
    x0, y0 = np.arange(bw) * 16, np.arange(bh) * 16
    x1, y1 = np.minimum(x0 + 16, 50) - 1, np.minimum(y0 + 16, 40) - 1
    v = vec4.astype(int)
    crossing = (4 * x1[None, None, :] + v[..., 1] > 4 * 49) | (4 * x0[None, None, :] + v[..., 1] < 0) | (4 * y1[None, :, None] + v[..., 0] > 4 * 39) | \
        (4 * y0[None, :, None] + v[..., 0] < 0)
    assert crossing.sum() >= 8 and np.abs(vec).max() == 16
    assert ref.refine_case("random", 17, 33, 16, 2, 0, 3)[3].shape == (3, 2, 3, 2)


# ---- warp -----------------------------------------------------------------------------------------------------------------------------------------
def _warp_inputs(h, w, block, seed, whole=False):
    rs = np.random.RandomState(seed)
    bh, bw, _ = ref.grid(h, w, block)
    vec4 = rs.choice([-67, 66, 0, 1, -3, 4 * rs.randint(-16, 17), rs.randint(-70, 71)], size=(bh, bw, 2)).astype(np.int16)
    if whole:
        vec4 = (4 * rs.randint(-16, 17, (bh, bw, 2))).astype(np.int16)
    return vec4, rs.randint(0, 256, (h, w, 3), dtype=np.uint8), rs.normal(0, 100, (h, w, 6)).astype(np.float32)


def _assert_warp(got_p, got_s, vec4, prev, state, block, what):
    want_p, want_s = ref.warp(vec4, prev, state, block)
    assert got_p.dtype == torch.uint8 and got_s.dtype == torch.float32 and same(got_p, want_p), what
    err = np.abs(got_s.cpu().numpy().astype(np.float64) - want_s)
    bound = STATE_BOUND * ref.tap_magnitude(vec4, state, block)
    assert (err <= bound).all(), (what, float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("block", ref.BLOCKS)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_warp_against_the_restatement(h, w, block):
    worst = 0.0
    for seed in range(3):
        vec4, prev, state = _warp_inputs(h, w, block, h + w + block + seed)
        got_p, got_s = ops.motion_warp_subpel(dev(vec4), dev(prev), dev(state), block)
        worst = max(worst, _assert_warp(got_p, got_s, vec4, prev, state, block, seed))
    print("warped state, %d x %d block %d: worst error %.3f of the bound" % (h, w, block, worst))
    vec4, prev, state = _warp_inputs(h, w, block, h + w, whole=True)
    tv, tp, ts = dev(vec4), dev(prev), dev(state)
    got_p, got_s = ops.motion_warp_subpel(tv, tp, ts, block)
    want_p, want_s = ops.motion_warp(dev(vec4 // 4), tp, ts, block)
    assert torch.equal(got_p, want_p) and torch.equal(got_s, want_s)            # multiples of 4: the whole-pixel warp, bit for bit
    zero_p, zero_s = ops.motion_warp_subpel(torch.zeros_like(tv), tp, ts, block)
    assert torch.equal(zero_p, tp) and torch.equal(zero_s, ts)                  # a zero field is a copy


# ---- unaligned buffers, a side stream, batching -----------------------------------------------------------------------------------------------------
def test_byte_offsets_and_a_side_stream():
    """guide, prev_guide and prev_out each 1 .. 3 bytes past a 16-byte boundary, and both calls on a side stream: the same results"""
    h, w, block, Q = 17, 33, 8, 4
    guide, prev, vec, vec4, sad4 = ref.refine_case("subshift", h, w, block, Q, BIAS, 3)
    wvec, wprev, wstate = _warp_inputs(h, w, block, 9)
    want_p, _ = ref.warp(wvec, wprev, wstate, block)
    tvec, tv, ts = dev(vec), dev(wvec), dev(wstate)
    _, want_s = ops.motion_warp_subpel(tv, dev(wprev), ts, block)
    _assert_warp(dev(want_p), want_s, wvec, wprev, wstate, block, "aligned")
    for k in (1, 2, 3):
        for ks in ((k, 0), (0, k), (k, (k + 1) % 4)):
            v, s = ops.motion_refine_u8(_at_offset(guide, ks[0]), _at_offset(prev, ks[1]), tvec, block, Q, BIAS)
            assert same(v, vec4) and same(s, sad4), ks
            out = (_at_offset(np.zeros((h, w, 3), np.uint8), ks[1]), torch.empty(h, w, 6, device=DEV))
            p, st = ops.motion_warp_subpel(tv, _at_offset(wprev, ks[0]), ts, block, out=out)
            assert p.data_ptr() == out[0].data_ptr() and same(p, want_p) and torch.equal(st, want_s), ks
    tg, tp, twp = dev(guide), dev(prev), dev(wprev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        v, s = ops.motion_refine_u8(tg, tp, tvec, block, Q, BIAS)
        p, st = ops.motion_warp_subpel(tv, twp, ts, block)
    side.synchronize()
    assert same(v, vec4) and same(s, sad4) and same(p, want_p) and torch.equal(st, want_s)


def test_one_call_on_four_frames_is_four_calls_of_one():
    f = dev(ref.subshift(40, 50, 4, 4, 6))
    vec, _ = ops.motion_search_u8(f[1:], f[0], 16, 3, BIAS)
    vec4, sad4 = ops.motion_refine_u8(f[1:], f[0], vec, 16, 4, BIAS)
    for k in range(4):
        v1, s1 = ops.motion_refine_u8(f[k + 1:k + 2], f[k], vec[k:k + 1], 16, 4, BIAS)
        assert torch.equal(v1[0], vec4[k]) and torch.equal(s1[0], sad4[k]), k
    for _ in range(2):                                           # repeated calls
        v, s = ops.motion_refine_u8(f[1:], f[0], vec, 16, 4, BIAS)
        assert torch.equal(v, vec4) and torch.equal(s, sad4)
    assert ref.fractional_share(vec4.cpu().numpy()) >= 0.5


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_subpel():
    """every input between 0xff bands, every output between random bands, prefilled 0xff, zeros and random bytes, for both entry points: no band
    changes, and the payload is the restatement's whatever it held before"""
    lib = _lib.load()
    for (h, w), block, Q in (((17, 33), 8, 4), ((40, 50), 32, 2), ((5, 7), 16, 4), ((40, 50), 16, 4)):
        guide, prev, vec, vec4, sad4 = ref.refine_case("subshift", h, w, block, Q, BIAS, 3, (h, w) == (17, 33))
        wvec, wprev, wstate = _warp_inputs(h, w, block, 3)
        tg, tp, tvec = guarded.guarded_copy(dev(guide)), guarded.guarded_copy(dev(prev)), guarded.guarded_copy(dev(vec))
        tv, twp, tws = guarded.guarded_copy(dev(wvec)), guarded.guarded_copy(dev(wprev)), guarded.guarded_copy(dev(wstate))
        ov = guarded.guarded_empty(vec4.shape, torch.int16, DEV)
        os_ = guarded.guarded_empty(sad4.shape, torch.int32, DEV)
        op = guarded.guarded_empty((h, w, 3), torch.uint8, DEV)
        ost = guarded.guarded_empty((h, w, 6), torch.float32, DEV)
        first = None
        for fill in guarded.FILLS:
            for t in (ov, os_, op, ost):
                guarded.refill(t, fill)
            _lib.check(lib.cfen_motion_refine_u8(_lib.ptr(tg), _lib.ptr(tp), _lib.ptr(tvec), 3, h, w, block, Q, BIAS, _lib.ptr(ov), _lib.ptr(os_),
                                                 _lib.current_stream()), "motion_refine_u8")
            _lib.check(lib.cfen_motion_warp_subpel(_lib.ptr(tv), _lib.ptr(twp), _lib.ptr(tws), h, w, block, _lib.ptr(op), _lib.ptr(ost),
                                                   _lib.current_stream()), "motion_warp_subpel")
            torch.cuda.synchronize()
            guarded.check_bands(tg, tp, tvec, ov, os_, tv, twp, tws, op, ost)
            assert same(ov, vec4) and same(os_, sad4), (h, w, fill)
            _assert_warp(op, ost, wvec, wprev, wstate, block, (h, w, fill))
            first = ost.clone() if first is None else first
            assert torch.equal(ost, first), (h, w, fill)         # the same bits whatever the output held before


def test_argument_errors_launch_nothing():
    h, w = 20, 20
    f = dev(motion_ref.frames("random", h, w, 2, 1))
    vec = torch.zeros((2, 3, 3, 2), dtype=torch.int16, device=DEV)
    vec4 = torch.full((2, 3, 3, 2), 7, dtype=torch.int16, device=DEV)
    sad4 = torch.full((2, 3, 3), 7, dtype=torch.int32, device=DEV)
    for bad in ({"block": 12}, {"block": 8.5}, {"subpel": 1}, {"subpel": 3}, {"subpel": 2.5}, {"subpel": 8}, {"bias": -1}, {"bias": 256}):
        with pytest.raises(ValueError, match="motion_refine_u8: (block|subpel|bias)"):
            ops.motion_refine_u8(f[1:], f[0], vec, **dict({"block": 8, "subpel": 2, "bias": 4}, **bad), out=(vec4, sad4))
    with pytest.raises(ValueError, match="needs prev_guide"):
        ops.motion_refine_u8(f[1:], f[0, :10], vec, 8, 2, 4)
    with pytest.raises(ValueError, match="needs vec"):
        ops.motion_refine_u8(f[1:], f[0], vec[:1], 8, 2, 4, out=(vec4, sad4))
    with pytest.raises(ValueError, match="needs vec"):
        ops.motion_refine_u8(f[1:], f[0], vec.int(), 8, 2, 4, out=(vec4, sad4))
    with pytest.raises(ValueError, match="out must be"):
        ops.motion_refine_u8(f[1:], f[0], vec, 8, 2, 4, out=(vec4[:1], sad4))
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_refine_u8(f[1:], f[1], vec, 8, 2, 4, out=(vec4, sad4))
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_refine_u8(f[1:], f[0], vec4, 8, 2, 4, out=(vec4, sad4))
    state = torch.full((h, w, 6), 7.0, device=DEV)
    out = (torch.full((h, w, 3), 9, dtype=torch.uint8, device=DEV), torch.full((h, w, 6), 9.0, device=DEV))
    with pytest.raises(ValueError, match="motion_warp_subpel needs vec4"):
        ops.motion_warp_subpel(vec4[0, :2], f[0], state, 8, out=out)
    with pytest.raises(ValueError, match="motion_warp_subpel needs state"):
        ops.motion_warp_subpel(vec4[0], f[0], state[:4], 8, out=out)
    with pytest.raises(ValueError, match="motion_warp_subpel: block"):
        ops.motion_warp_subpel(vec4[0], f[0], state, 4, out=out)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_warp_subpel(vec4[0], f[0], state, 8, out=(f[0], out[1]))
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.motion_warp_subpel(vec4[0], f[0], state, 8, out=(out[0], state))
    torch.cuda.synchronize()
    assert bool((vec4 == 7).all()) and bool((sad4 == 7).all()) and bool((out[0] == 9).all()) and bool((out[1] == 9.0).all()) and bool((state == 7.0).all())


# ---- the compensated recursion ---------------------------------------------------------------------------------------------------------------------
def _compose(tG, tY, Q, radius=2, eps=1e-4, strength=0.8, motion=8.0, down=1, mc_range=4, mc_block=16, mc_bias=BIAS):
    """the refined Stabiliser written out with the operators, frame by frame: (frames, state, every vec4)"""
    n, H, W, _ = tG.shape
    S, h, w = temporal.working_size(H, W, down)
    I, P = (tG, tY) if S == 1 else (ops.resample_u8(tG, (h, w), filter="box"), ops.resample_u8(tY, (h, w), filter="box"))
    coef = ops.guided_coef_u8(I, P, radius, eps)
    state = torch.empty(h, w, 6, device=DEV)
    deltas, fields = [ops.temporal_blend(I[:1], None, coef[:1], state, radius, motion, strength, False)], []
    for k in range(1, n):
        vec, _ = ops.motion_search_u8(I[k:k + 1], I[k - 1], mc_block, mc_range, mc_bias)
        vec4, _ = ops.motion_refine_u8(I[k:k + 1], I[k - 1], vec, mc_block, Q, mc_bias)
        warped, state = ops.motion_warp_subpel(vec4[0], I[k - 1], state, mc_block)
        deltas.append(ops.temporal_blend(I[k:k + 1], warped, coef[k:k + 1].clone(), state, radius, motion, strength, True))          # (a 16-byte aligned copy)
        fields.append(vec4[0])
    return ops.temporal_apply_u8(torch.cat(deltas), tG, tY), state, torch.stack(fields)


def _clip(n, H, W, Q, seed):
    """hazy frames of a gentle texture that moves by a fraction of a pixel per frame (gain 1: an aligned block passes the blend's motion test), and
    flickering outputs"""
    G = ref.subshift(H, W, n - 1, Q, seed, gain=1.0)
    rs = np.random.RandomState(seed)
    Y = np.clip(0.9 * G + rs.normal(0, 6, (n, 1, 1, 3)) + rs.randint(-2, 3, G.shape) - 20, 0, 255).astype(np.uint8)
    return G, Y


@pytest.mark.parametrize("Q", ref.SUBPELS)
@pytest.mark.parametrize("H,W,down,block", [(40, 64, 1, 16), (75, 101, 2, 8), (45, 71, 1, 32)])          # the last: odd h w, frames of a batch 8 bytes off
def test_stabiliser_is_the_composition_of_its_operators_and_does_not_depend_on_batching(H, W, down, block, Q):
    G, Y = _clip(5, H, W, Q, H + Q)
    tG, tY = dev(G), dev(Y)
    want, state, fields = _compose(tG, tY, Q, down=down, mc_block=block)
    whole = temporal.Stabiliser(down=down, mc_range=4, mc_block=block).step(tG, tY)
    assert torch.equal(want[0], tY[0])
    if down == 1:
        assert bool((fields & 3).any()) and not torch.equal(want, whole)       # the field is fractional: refinement changes the bytes
    for sizes in ((5,), (1, 1, 1, 1, 1), (2, 2, 1), (1, 4), (3, 2)):                      # batches of 1, 2 and 5, and mixtures
        st = temporal.Stabiliser(down=down, mc_range=4, mc_block=block, mc_subpel=Q)
        parts, lo = [], 0
        for m in sizes:
            parts.append(st.step(tG[lo:lo + m], tY[lo:lo + m]))
            lo += m
        assert torch.equal(torch.cat(parts), want) and torch.equal(st._state, state), sizes
    st.reset()
    assert st._vec4 is None and st._sad4 is None and st._vec is None
    out = torch.empty_like(tY)
    assert st.step(tG, tY, out=out).data_ptr() == out.data_ptr() and torch.equal(out, want)


@pytest.mark.parametrize("Q", ref.SUBPELS)
def test_the_refined_recursion_against_float64(Q):
    """given coefficients, four frames of a texture that moves by fractions of a pixel: the device's search -> refine -> warp -> blend (B = 1) chain
    against the float64 restatement of the same chain; Delta and S within TAU_T, the bytes by assert_bytes"""
    h, w, block, R, r = 40, 50, 16, 3, 2
    f = ref.subshift(h, w, 3, Q, 12, gain=1.0)
    coef = temporal_ref.coefficients(4, h, w, 12) * np.float32(0.1)
    Y = np.random.RandomState(12).randint(0, 256, f.shape, dtype=np.uint8)
    tf, tc = dev(f), dev(coef)
    state = torch.full((h, w, 6), float("nan"), device=DEV)
    deltas = [ops.temporal_blend(tf[:1], None, tc[:1], state, r, temporal_ref.MOTION, temporal_ref.STRENGTH, False)]
    d64, s64, _, _ = temporal_ref.blend(f[:1], None, coef[:1], r, temporal_ref.MOTION, temporal_ref.STRENGTH, None)
    want = [d64[0]]
    kept = fractional = 0
    for k in range(1, 4):
        vec, _ = ops.motion_search_u8(tf[k:k + 1], tf[k - 1], block, R, BIAS)
        vec4, _ = ops.motion_refine_u8(tf[k:k + 1], tf[k - 1], vec, block, Q, BIAS)
        warped, state = ops.motion_warp_subpel(vec4[0], tf[k - 1], state, block)
        deltas.append(ops.temporal_blend(tf[k:k + 1], warped, tc[k:k + 1], state, r, temporal_ref.MOTION, temporal_ref.STRENGTH, True))
        v64 = ref.refine_one(f[k], f[k - 1], motion_ref.search_one(f[k], f[k - 1], block, R, BIAS)[0], block, Q, BIAS)[0]
        assert same(vec4[0], v64)
        fractional += int((v64 & 3).any())
        p64, sw64 = ref.warp(v64, f[k - 1], s64, block)
        assert same(warped, p64)
        d64, s64, keep, _ = temporal_ref.blend(f[k:k + 1], p64, coef[k:k + 1], r, temporal_ref.MOTION, temporal_ref.STRENGTH, sw64)
        want.append(d64[0])
        kept += int((keep > 0).sum())
    assert kept and fractional == 3                              # the recursion was on somewhere, along fractional vectors
    delta = torch.cat(deltas)
    ed = np.abs(delta.cpu().numpy().astype(np.float64) - np.stack(want)).max()
    es = np.abs(state.cpu().numpy().astype(np.float64) - s64).max()
    print("refined chain, Q = %d: max |dDelta| %.3e, |dS| %.3e (TAU_T %.3e), keep > 0 on %d pixel-frames" % (Q, ed, es, TAU_T, kept))
    assert ed <= TAU_T and es <= TAU_T
    got = ops.temporal_apply_u8(delta, tf, dev(Y)).cpu().numpy()
    assert_bytes(got, np.stack([temporal_ref.apply_v(want[k], f[k], Y[k]) for k in range(4)]), "refined chain")


def test_identical_hazy_frames_equal_the_whole_pixel_run():
    """SAD4(0) = 0 wins every tie: the refined field is zero, the warp a copy, and mc_subpel 2 and 4 are mc_subpel 1 and mc_range 0 bit for bit"""
    G, Y = _clip(4, 45, 70, 4, 3)
    tG, tY = dev(G[:1]).repeat(4, 1, 1, 1), dev(Y)
    for down in (1, 2):
        want = temporal.Stabiliser(down=down).step(tG, tY)
        assert not torch.equal(want, tY)
        for block in ref.BLOCKS:
            assert torch.equal(temporal.Stabiliser(down=down, mc_range=4, mc_block=block, mc_bias=0).step(tG, tY), want)
            for Q in ref.SUBPELS:
                st = temporal.Stabiliser(down=down, mc_range=4, mc_block=block, mc_bias=0, mc_subpel=Q)
                assert torch.equal(st.step(tG, tY), want) and not bool(st._vec4[:3].any()) and not bool(st._sad4[:3].any())


def test_the_fractional_pan_flickers_less_on_the_device():
    """the first clip of DESIGN section 25 (192 x 256, (1, 3) pixels per frame, stabilised at 96 x 128): the device's frames at mc_subpel 1, 2 and 4
    against the float64 restatement's by the bar of test_hip_motion.test_the_panning_clip_flickers_less_on_the_device (a byte differs by at most
    1, on fewer than one byte in a hundred), so the flicker along the motion agrees within twice that share; and refinement brings it below the
    whole-pixel device run's by the bar of tests/test_subpel_host.py"""
    from test_subpel_host import HALF_BAR
    G, Y, J, origin = ref.clip("half")
    down = ref.CLIPS["half"][3]
    tG, tY = dev(G), dev(Y)
    figures = {}
    for Q in (1, 2, 4):
        got = temporal.Stabiliser(down=down, mc_range=motion_ref.PAN_RANGE, mc_subpel=Q).step(tG, tY).cpu().numpy()
        want = ref.clip_run("half", Q)
        diff = np.abs(got.astype(np.int64) - want)
        share = (diff != 0).mean()
        fl, fl_ref = motion_ref.flicker_along_motion(got, origin), motion_ref.flicker_along_motion(want, origin)
        figures[Q] = {"flicker_device": fl, "flicker_restatement": fl_ref, "psnr_device": motion_ref.psnr(got[4:], J[4:]),
                      "bytes_differing": int((diff != 0).sum()), "bytes": int(diff.size)}
        print("mc_subpel %d: flicker along the motion, device %.3f, restatement %.3f; %d of %d bytes differ" % (Q, fl, fl_ref, (diff != 0).sum(), diff.size))
        assert diff.max() <= 1 and share < 0.01, Q
        assert abs(fl - fl_ref) <= 2 * share + 1e-12, Q
    assert figures[2]["flicker_device"] <= HALF_BAR * figures[1]["flicker_device"]
    assert figures[4]["psnr_device"] >= figures[1]["psnr_device"] and figures[2]["psnr_device"] >= figures[1]["psnr_device"]
    if os.environ.get("CFEN_WRITE_PARITY") == "1":
        with open(os.path.join(ROOT, "profiles", "subpel_parity.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "clip": "192 x 256, (1, 3) pixels per frame, down 2, range 4, block 16, bias 4",
                       "bar": "a byte differs by at most 1, on fewer than 1 in 100; flicker within twice that share", "mc_subpel": figures}, f, indent=1,
                      sort_keys=True)
            f.write("\n")


# ---- dehaze_video.py --temporal_mc_subpel ------------------------------------------------------------------------------------------------------------
def _shifting_stream(n, H, W, chroma, seed=23):
    """a y4m stream of a smooth texture that moves by half pixels per frame, and the frames' RGB by the restatement"""
    G = ref.subshift(H, W, n - 1, 2, seed, gain=1.0)
    frames = [yuv_ref.rgb_to_yuv(g, chroma, "bt601", False) for g in G]
    header = yuv_ref.y4m_header(W, H, chroma)
    return yuv_ref.y4m_bytes(frames, W, H, chroma, header=header), header, [yuv_ref.yuv_to_rgb(f, H, W, chroma, "bt601", False) for f in frames]


@pytest.mark.parametrize("route", list(CLIPS))
def test_cli_temporal_mc_subpel(route, tmp_path, ckpt):
    """dehaze_video.py --temporal --temporal_mc 4 --temporal_mc_subpel 2 in a child process: the stream is, bit for bit, library route ->
    Stabiliser(mc_range=4, mc_subpel=2).step -> the restatement's RGB -> YCbCr; the same clip without the flag is the whole-pixel Stabiliser's,
    as before, and prints and records nothing new.  The 1.9 GB checkpoint is test_hip_video_deep's shared one: this module leaves no copy behind"""
    import test_hip_video as vid
    import test_hip_video_deep as deep
    n, H, W, chroma, flags = CLIPS[route]
    data, header, rgb = _shifting_stream(n, H, W, chroma)
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
    st, whole = temporal.Stabiliser(mc_range=4, mc_subpel=2), temporal.Stabiliser(mc_range=4)
    fine = torch.cat([st.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
    coarse = torch.cat([whole.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
    assert torch.equal(fine[0], y[0]) and not torch.equal(fine, coarse)
    print("%s: refinement changes %.1f %% of the bytes of the whole-pixel run" % (route, 100 * (fine != coarse).float().mean().item()))

    def check(out_bytes, want):
        got_header, got = yuv_ref.y4m_frames(out_bytes, H, W, chroma)
        assert got_header == header and len(got) == n
        for k in range(n):
            assert np.array_equal(got[k], yuv_ref.rgb_to_yuv(want[k], chroma, "bt601", False)), (route, k)

    mc = ["--batchSize", "2", "--temporal", "--temporal_mc", "4"]
    r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", tmp_path / "fine.y4m", flags + mc + ["--temporal_mc_subpel", "2"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    text = r.stdout.decode()
    assert "temporal_mc_subpel: 2" in text and "video: vectors refined to 1/2 pixel" in text and "video: motion compensation within +-4 pixels" in text
    assert "temporal_mc_subpel: 2" in (ckpt / deep.NAME / "video_opt.txt").read_text()
    check((tmp_path / "fine.y4m").read_bytes(), fine.cpu().numpy())
    r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", tmp_path / "coarse.y4m", flags + mc)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "subpel" not in r.stdout.decode().replace(str(tmp_path), "") and "vectors refined" not in r.stdout.decode()
    assert "subpel" not in (ckpt / deep.NAME / "video_opt.txt").read_text().replace(str(tmp_path), "")
    check((tmp_path / "coarse.y4m").read_bytes(), coarse.cpu().numpy())
    if route == "plain":                                       # a refusal leaves with 2, names the flag and writes nothing
        for extra in (["--temporal", "--temporal_mc", "4", "--temporal_mc_subpel", "3"], ["--temporal", "--temporal_mc_subpel", "2"],
                      ["--temporal_mc_subpel", "2"]):
            r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", tmp_path / "none.y4m", extra)
            assert r.returncode == 2 and b"--temporal_mc_subpel" in r.stderr and not (tmp_path / "none.y4m").exists(), extra
