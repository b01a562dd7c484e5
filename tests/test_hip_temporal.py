"""Temporal stabilisation on the device (cfen_temporal_blend, cfen_temporal_apply_u8; ops.temporal_blend, ops.temporal_apply_u8,
temporal.Stabiliser, dehaze_video.py --temporal).  The reference is the float64 restatement tests/temporal_ref.py; the tolerance TAU_T is measured
on the CPU in tests/test_temporal_host.py, never against the kernels; the determinism, composition and end-to-end tests have no tolerance."""
import os

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, ops, temporal
import guarded
import guided_ref
import temporal_ref as ref
import yuv_ref
from test_temporal_host import TAU_T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared reference arrays are read-only


def run_blend(guide, prev, coef, state0, r, motion=ref.MOTION, strength=ref.STRENGTH):
    """(delta, state) of one call; state0 None: the first frame of a stream, the state tensor prefilled with NaN"""
    h, w = guide.shape[1:3]
    state = dev(state0) if state0 is not None else torch.full((h, w, 6), float("nan"), device=DEV)
    delta = ops.temporal_blend(dev(guide), dev(prev) if state0 is not None else None, dev(coef), state, r, motion, strength, state0 is not None)
    return delta, state


# ---- blend --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("have_state", [False, True], ids=["first", "carried"])
@pytest.mark.parametrize("B", ref.BATCHES)
@pytest.mark.parametrize("r", ref.RADII)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_blend_against_float64(h, w, r, B, have_state):
    guide, prev, coef, state0, delta64, state64, keep64, D = ref.blend_case(h, w, r, B, have_state)
    delta, state = run_blend(guide, prev, coef, state0, r)
    assert delta.shape == (B, h, w, 6) and delta.dtype == torch.float32
    d, s = delta.cpu().numpy(), state.cpu().numpy()
    ed, es = np.abs(d.astype(np.float64) - delta64).max(), np.abs(s.astype(np.float64) - state64).max()
    print("%dx%d r %d B %d %s: max |dDelta| %.3e, |dS| %.3e (TAU_T %.3e); keep 0 on %d, 1 on %d, between on %d pixel-frames"
          % (h, w, r, B, have_state, ed, es, TAU_T, (keep64 == 0).sum(), (keep64 == 1).sum(), ((keep64 > 0) & (keep64 < 1)).sum()))
    assert np.isfinite(d).all() and np.isfinite(s).all() and ed <= TAU_T and es <= TAU_T
    # keep is exactly 0 where D says so (3 N motion <= D, in integers; and the first frame of a stream): Delta = 0 and S = c, bit for bit
    N = guided_ref.window_count(h, w, r)
    off = (D >= 3 * N * int(ref.MOTION)) | (D < 0)
    assert not d[off].any()
    assert np.array_equal(s[off[-1]], coef[-1][off[-1]])


def test_keep_is_exactly_0_and_1_where_the_motion_sum_says_so():
    """coefficients on a grid of 1/4 and strength 1/2: every operation of the recursion is exact in fp32 whether or not multiply and add are fused,
    so wherever every frame so far had D = 0 (keep = 1) or D >= 3 N motion (keep = 0) the device's Delta and S are the float64 ones, bit for bit"""
    h, w, r, B = 40, 50, 2, 4
    seen, partial = set(), 0
    for seed in (0, 1, 2, 3):
        f = ref.frames(h, w, B, seed)
        coef = (np.random.RandomState(seed).randint(-32, 33, (B, h, w, 6)) / 4.0).astype(np.float32)
        delta64, state64, keep64, D = ref.blend(f[1:], None, coef, r, 8.0, 0.5)
        N = guided_ref.window_count(h, w, r)
        exact = np.zeros(D.shape, bool)                        # a pixel with keep = 0 is exact whatever came before it: S = c
        for k in range(B):
            exact[k] = (D[k] < 0) | (D[k] >= 24 * N) | ((D[k] == 0) & exact[k - 1])
        seen |= set(np.unique(keep64[exact]))
        partial += int((~exact).sum())
        delta, state = run_blend(f[1:], None, coef, None, r, 8.0, 0.5)
        d, s = delta.cpu().numpy(), state.cpu().numpy()
        assert np.array_equal(d[exact].astype(np.float64), delta64[exact]) and np.array_equal(s[exact[-1]].astype(np.float64), state64[exact[-1]])
    assert seen == {0.0, 1.0} and partial


# ---- apply ----------------------------------------------------------------------------------------------------------------------------------------
def assert_bytes(got, v64, what):
    """a byte may differ from the reference's, by exactly 1, only where the reference's v lies within TAU_T of k + 0.5"""
    want = ref.to_bytes(v64)
    assert got.shape == want.shape and got.dtype == np.uint8
    diff = got.astype(np.int64) - want
    dist = np.abs((v64 - 0.5) - np.round(v64 - 0.5))             # distance of v to the nearest k + 0.5
    print("%s: %d of %d bytes differ, %d lie within TAU_T of a rounding boundary" % (what, (diff != 0).sum(), diff.size, (dist <= TAU_T).sum()))
    assert np.abs(diff).max() <= 1, what
    assert (dist[diff != 0] <= TAU_T).all(), (what, float(dist[diff != 0].max()))


def test_paths_the_cases_claim():
    """row pitches that send a case to the 16-byte or the byte path, and the column counts that send a workgroup to the staged (<= 1024 columns)
    or the global-memory path"""
    pitch = {n: 3 * c[1][1] for n, c in ref.APPLY_CASES.items()}
    assert sorted(n for n, p in pitch.items() if p % 16 == 0) == ["2x1376_1to1", "3x344_2x1376", "40x32_1to1"]
    assert sorted(n for n, p in pitch.items() if p > 4096) == ["2x1376_1to1", "2x1400_1to1", "3x344_2x1376", "3x350_2x1400"]

    def columns(w, W, first, last):
        x0, x1, _ = guided_ref.axis_coords(w, W)
        return int(x1[min(last, W - 1)] - x0[first] + 1)
    assert columns(1400, 1400, 0, 1365) == 1367 and columns(1376, 1376, 0, 1365) == 1367             # more than are staged
    assert columns(350, 1400, 0, 1365) <= 1024 and columns(344, 1376, 0, 1365) <= 1024 and columns(1400, 1400, 1365, 1399) <= 1024
    assert columns(960, 3840, 0, 1365) == 342                                                         # a 2160 x 3840 frame at down = auto


@pytest.mark.parametrize("name", list(ref.APPLY_CASES))
def test_apply_against_float64(name):
    delta, G, Y, v64 = ref.apply_case(name)
    got = ops.temporal_apply_u8(dev(delta), dev(G), dev(Y))
    assert got.shape == G.shape and got.dtype == torch.uint8
    g = got.cpu().numpy()
    assert_bytes(g, v64, name)
    h, w = delta.shape[1:3]
    H, W = G.shape[1:3]
    if (h, w) == (H, W):                                       # where delta is 0 (a block of every case) the bytes are src_hi's
        assert np.array_equal(g[:, : (h + 1) // 2 - 1, : (w + 1) // 2 - 1], Y[:, : (h + 1) // 2 - 1, : (w + 1) // 2 - 1])
    assert not np.array_equal(g, Y)


def _at_offset(a, k):
    """a contiguous device copy of `a` that starts k bytes past a 16-byte boundary"""
    buf = torch.empty(a.size + 32, dtype=torch.uint8, device=DEV)
    lead = (-buf.data_ptr()) % 16 + k
    t = buf[lead:lead + a.size].view(a.shape)
    t.copy_(dev(a))
    assert t.data_ptr() % 16 == k and t.is_contiguous()
    return t


@pytest.mark.parametrize("name", ["13x21_37x61", "40x32_1to1", "2x1376_1to1"])
def test_apply_at_byte_offsets(name):
    """guide_hi, src_hi and dst each 1 .. 3 bytes past a 16-byte boundary: the same bytes as with all three aligned"""
    delta, G, Y, _ = ref.apply_case(name)
    td = dev(delta)
    want = ops.temporal_apply_u8(td, dev(G), dev(Y))
    for which in range(3):
        for k in (1, 2, 3):
            ks = [k if which == i else 0 for i in range(3)]
            out = _at_offset(np.zeros(G.shape, np.uint8), ks[2])
            got = ops.temporal_apply_u8(td, _at_offset(G, ks[0]), _at_offset(Y, ks[1]), out=out)
            assert got.data_ptr() == out.data_ptr() and torch.equal(got, want), (which, k)


# ---- determinism and the exact properties -----------------------------------------------------------------------------------------------------------
def _clip(n, H, W, seed):
    """hazy and dehazed frames (n, H, W, 3) of a slowly changing scene: identical, noisy and locally changed neighbours, no cut"""
    rs = np.random.RandomState(seed)
    base = rs.randint(0, 256, (H, W, 3))
    G = np.stack([np.clip(base + rs.randint(-3, 4, base.shape), 0, 255) for _ in range(n)]).astype(np.uint8)
    Y = np.clip(0.9 * G + rs.normal(0, 6, (n, 1, 1, 3)) + rs.randint(-2, 3, G.shape) - 20, 0, 255).astype(np.uint8)
    G[2] = G[1]                                                # one identical pair of hazy frames
    return G, Y


@pytest.mark.parametrize("H,W,down", [(37, 53, 1), (40, 64, 1), (75, 101, 2)])
def test_one_call_on_four_frames_is_four_calls_of_one(H, W, down):
    G, Y = _clip(4, H, W, H + W)
    tG, tY = dev(G), dev(Y)
    whole = temporal.Stabiliser(down=down).step(tG, tY)
    assert whole.shape == (4, H, W, 3) and torch.equal(whole[0], tY[0]) and not torch.equal(whole[1:], tY[1:])
    one = temporal.Stabiliser(down=down)
    for k in range(4):
        assert torch.equal(one.step(tG[k:k + 1], tY[k:k + 1]), whole[k:k + 1]), k
    mixed = temporal.Stabiliser(down=down)                     # 1 + 3
    assert torch.equal(torch.cat([mixed.step(tG[:1], tY[:1]), mixed.step(tG[1:], tY[1:])]), whole)
    for _ in range(2):                                         # repeated calls
        assert torch.equal(temporal.Stabiliser(down=down).step(tG, tY), whole)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = temporal.Stabiliser(down=down).step(tG, tY)
    side.synchronize()
    assert torch.equal(on_side, whole)
    st = temporal.Stabiliser(down=down)                        # reset() starts a new stream; out= is used
    st.step(tG[2:], tY[2:])
    st.reset()
    out = torch.empty_like(tY)
    assert st.step(tG, tY, out=out).data_ptr() == out.data_ptr() and torch.equal(out, whole)


def test_the_raw_calls_do_not_depend_on_batching_or_on_what_the_outputs_held():
    h, w, H, W, r, B = 17, 33, 37, 61, 2, 3
    guide, prev, coef, state0, _, _, _, _ = ref.blend_case(17, 33, 2, 3, True)
    delta, state = run_blend(guide, prev, coef, state0, r)
    rs = np.random.RandomState(5)
    G, Y = dev(rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8)), dev(rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8))
    dst = ops.temporal_apply_u8(delta, G, Y)
    s = dev(state0)
    for k in range(B):                                         # B = 3 equals three B = 1 calls with carried state
        dk = ops.temporal_blend(dev(guide[k:k + 1]), dev(guide[k - 1] if k else prev), dev(coef[k:k + 1]), s, r, ref.MOTION, ref.STRENGTH, True)
        assert torch.equal(dk, delta[k:k + 1]), k
        assert torch.equal(ops.temporal_apply_u8(dk, G[k:k + 1], Y[k:k + 1]), dst[k:k + 1]), k
    assert torch.equal(s, state)
    lib = _lib.load()
    tg, tp, tc = dev(guide), dev(prev), dev(coef)
    for fill in ("zero", "ff", "random"):                      # what delta and dst held before does not matter
        d2 = guarded.guarded_empty((B, h, w, 6), torch.float32, DEV, fill=fill)
        o2 = guarded.guarded_empty((B, H, W, 3), torch.uint8, DEV, fill=fill)
        s2 = dev(state0)
        _lib.check(lib.cfen_temporal_blend(_lib.ptr(tg), _lib.ptr(tp), _lib.ptr(tc), B, h, w, r, ref.MOTION, ref.STRENGTH, 1, _lib.ptr(s2), _lib.ptr(d2),
                                           _lib.current_stream()), "temporal_blend")
        _lib.check(lib.cfen_temporal_apply_u8(_lib.ptr(d2), B, h, w, _lib.ptr(G), _lib.ptr(Y), H, W, _lib.ptr(o2), _lib.current_stream()), "temporal_apply_u8")
        assert torch.equal(d2, delta) and torch.equal(s2, state) and torch.equal(o2, dst), fill
    for fill in (0.0, float("nan"), 1e30):                     # have_state = 0: what state held before does not matter either
        s3 = torch.full((h, w, 6), fill, device=DEV)
        d3 = ops.temporal_blend(tg, None, tc, s3, r, ref.MOTION, ref.STRENGTH, False)
        want_d, want_s = run_blend(guide, prev, coef, None, r)
        assert torch.equal(d3, want_d) and torch.equal(s3, want_s) and not d3[0].any()


@pytest.mark.parametrize("down", [1, 2])
def test_the_three_exact_consequences_on_the_device(down):
    G, Y = _clip(3, 45, 70, 9)
    tG, tY = dev(G), dev(Y)
    st = temporal.Stabiliser(down=down)                        # identical consecutive frames: dst == Y
    for _ in range(3):
        assert torch.equal(st.step(tG[:1], tY[:1]), tY[:1])
    assert torch.equal(temporal.Stabiliser(down=down).step(tG[:1].repeat(3, 1, 1, 1), tY[:1].repeat(3, 1, 1, 1)), tY[:1].repeat(3, 1, 1, 1))
    st = temporal.Stabiliser(down=down)                        # a cut: dst == Y, and the state is this frame's coefficients
    st.step(tG[:2], tY[:2])
    cut = dev((G[2].astype(np.int64) + 100).astype(np.uint8))[None]
    assert torch.equal(st.step(cut, tY[2:]), tY[2:])
    S, h, w = temporal.working_size(45, 70, down)
    I, P = (cut, tY[2:]) if S == 1 else (ops.resample_u8(cut, (h, w), filter="box"), ops.resample_u8(tY[2:], (h, w), filter="box"))
    assert torch.equal(st._state, ops.guided_coef_u8(I, P, 2, 1e-4)[0])
    st = temporal.Stabiliser(strength=0.0, down=down)          # strength 0: dst == Y for every input
    assert torch.equal(st.step(tG, tY), tY) and torch.equal(st.step(tG[:1], tY[1:2]), tY[1:2])


def test_stabiliser_is_the_composition_of_its_operators():
    G, Y = _clip(3, 75, 101, 4)
    tG, tY = dev(G), dev(Y)
    I, P = ops.resample_u8(tG, (38, 51), filter="box"), ops.resample_u8(tY, (38, 51), filter="box")
    coef = ops.guided_coef_u8(I, P, 3, 1e-3)
    state = torch.empty(38, 51, 6, device=DEV)
    delta = ops.temporal_blend(I, None, coef, state, 3, 4.0, 0.6, False)
    want = ops.temporal_apply_u8(delta, tG, tY)
    st = temporal.Stabiliser(radius=3, eps=1e-3, strength=0.6, motion=4.0, down=2)
    assert torch.equal(st.step(tG, tY), want) and torch.equal(st._state, state) and torch.equal(st._prev, I[2])
    # and against the restatement: a byte differs by at most 1 (the coefficients of step 2 carry the tolerance of tests/test_hip_guided.py)
    host = ref.Stabiliser(radius=3, eps=1e-3, strength=0.6, motion=4.0, down=2)
    ref_out = np.stack([host.step(G[k], Y[k])[0] for k in range(3)])
    diff = np.abs(want.cpu().numpy().astype(np.int64) - ref_out)
    print("against the restatement: %d of %d bytes differ, by at most %d" % ((diff != 0).sum(), diff.size, diff.max()))
    # the device's coefficients are within 1.29e-3 levels of the restatement's (test_guided_host.TAU), the recursion and the apply step within
    # TAU_T: a byte can flip only where v lies within a few 1e-3 of a rounding boundary, well under one byte in a hundred
    assert diff.max() <= 1 and (diff != 0).mean() < 0.01
    with pytest.raises(ValueError, match="reset"):
        st.step(tG[:, :40].contiguous(), tY[:, :40].contiguous())
    with pytest.raises(ValueError, match="differ in shape"):
        st.step(tG, tY[:2])
    with pytest.raises(ValueError, match="uint8 CUDA tensor"):
        st.step(tG.float(), tY)


# ---- guard bands, and argument errors --------------------------------------------------------------------------------------------------------------
def test_guard_bands_temporal():
    """every input between 0xff bands, state, delta and dst between random bands, for both entry points: no band changes, the results are the
    unguarded calls', whatever delta and dst held before; dst as lane 1 of a slab leaves the neighbouring lanes untouched"""
    lib = _lib.load()
    B, h, w, r = 3, 33, 40, 4
    f = ref.frames(h, w, B, 21)
    coef = ref.coefficients(B, h, w, 21)
    state0 = ref.coefficients(1, h, w, 22)[0]
    want_delta, want_state = run_blend(f[1:], f[0], coef, state0, r)
    tg, tp, tc = guarded.guarded_copy(dev(f[1:])), guarded.guarded_copy(dev(f[0])), guarded.guarded_copy(dev(coef))
    state = guarded.guarded_empty((h, w, 6), torch.float32, DEV, fill="ff")
    delta = guarded.guarded_empty((B, h, w, 6), torch.float32, DEV, fill="ff")
    for H, W in ((37, 53), (20, 1376)):                        # byte path; vector path with two workgroups per row
        rs = np.random.RandomState(H)
        G, Y = rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8), rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
        tG, tY = guarded.guarded_copy(dev(G)), guarded.guarded_copy(dev(Y))
        dst = guarded.guarded_empty((B, H, W, 3), torch.uint8, DEV, fill="ff")
        want = ops.temporal_apply_u8(want_delta, dev(G), dev(Y))
        for fill in ("ff", "zero"):
            for t in (delta, dst):
                guarded.refill(t, fill)
            for have in (0, 1):
                state.copy_(dev(state0))
                _lib.check(lib.cfen_temporal_blend(_lib.ptr(tg), _lib.ptr(tp), _lib.ptr(tc), B, h, w, r, ref.MOTION, ref.STRENGTH, have, _lib.ptr(state),
                                                   _lib.ptr(delta), _lib.current_stream()), "temporal_blend")
                torch.cuda.synchronize()
                guarded.check_bands(tg, tp, tc, state, delta)
                assert bool(torch.isfinite(delta).all()) and bool(torch.isfinite(state).all())
            assert torch.equal(delta, want_delta) and torch.equal(state, want_state), (H, W, fill)
            _lib.check(lib.cfen_temporal_apply_u8(_lib.ptr(delta), B, h, w, _lib.ptr(tG), _lib.ptr(tY), H, W, _lib.ptr(dst), _lib.current_stream()),
                       "temporal_apply_u8")
            torch.cuda.synchronize()
            guarded.check_bands(delta, tG, tY, dst)
            assert torch.equal(dst, want), (H, W, fill)
        assert_bytes(dst.cpu().numpy(), np.stack([ref.apply_v(want_delta[b].cpu().numpy(), G[b], Y[b]) for b in range(B)]), "guarded %d x %d" % (H, W))
        slab = dev(rs.randint(0, 256, (3, 1, H, W, 3), dtype=np.uint8))      # dst as lane 1 of a slab: at 37 x 53 the lane starts at an odd address
        before = slab.clone()
        ops.temporal_apply_u8(want_delta[:1], dev(G[:1]), dev(Y[:1]), out=slab[1])
        assert torch.equal(slab[1], want[:1]) and torch.equal(slab[0], before[0]) and torch.equal(slab[2], before[2])
        assert (slab[1].data_ptr() % 2 == 1) == ((H, W) == (37, 53))


def test_argument_errors_launch_nothing():
    h, w, H, W = 9, 11, 20, 30
    f = ref.frames(h, w, 2, 3)
    guide, prev, coef = dev(f[1:]), dev(f[0]), dev(ref.coefficients(2, h, w, 3))
    state = torch.full((h, w, 6), 7.0, device=DEV)
    delta = torch.full((2, h, w, 6), 7.0, device=DEV)
    for bad in ({"radius": 0}, {"radius": 17}, {"radius": 2.5}, {"motion": 0.0}, {"motion": float("nan")}, {"motion": float("inf")}, {"strength": 1.0},
                {"strength": -0.5}, {"strength": float("nan")}):
        with pytest.raises(ValueError, match="temporal_blend: (radius|motion|strength)"):
            ops.temporal_blend(guide, prev, coef, state, out=delta, **bad)
    with pytest.raises(ValueError, match="temporal_blend needs coef"):
        ops.temporal_blend(guide, prev, coef[:1], state)
    with pytest.raises(ValueError, match="temporal_blend needs state"):
        ops.temporal_blend(guide, prev, coef, state[:4])
    with pytest.raises(ValueError, match="needs prev_guide"):
        ops.temporal_blend(guide, None, coef, state)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.temporal_blend(guide, guide[0], coef, state, out=delta)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.temporal_blend(guide, prev, coef, coef[0], out=delta)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.temporal_blend(guide, prev, coef, state, out=coef)
    lib = _lib.load()
    s = _lib.current_stream()
    assert lib.cfen_temporal_blend(_lib.ptr(guide), _lib.ptr(prev), _lib.ptr(coef), 2, h, w, 2, 8.0, 1.0, 1, _lib.ptr(state), _lib.ptr(delta), s) == -1
    assert lib.cfen_temporal_blend(_lib.ptr(guide), _lib.ptr(prev), _lib.ptr(coef), 2, h, w, 2, 0.0, 0.5, 1, _lib.ptr(state), _lib.ptr(delta), s) == -1
    assert lib.cfen_temporal_blend(_lib.ptr(guide), None, _lib.ptr(coef), 2, h, w, 2, 8.0, 0.5, 1, _lib.ptr(state), _lib.ptr(delta), s) == -1
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((delta == 7.0).all())
    G, Y = dev(np.zeros((2, H, W, 3), np.uint8)), dev(np.ones((2, H, W, 3), np.uint8))
    dst = torch.full((2, H, W, 3), 9, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="temporal_apply_u8 needs delta"):
        ops.temporal_apply_u8(delta[..., :3].contiguous(), G, Y, out=dst)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.temporal_apply_u8(delta, G, Y[:1], out=dst)
    with pytest.raises(ValueError, match="temporal_apply_u8: out must be"):
        ops.temporal_apply_u8(delta, G, Y, out=dst.float())
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.temporal_apply_u8(delta, G, Y, out=Y)
    with pytest.raises(_lib.CfenError, match="must not overlap"):
        ops.temporal_apply_u8(delta, G, G, out=dst)
    assert lib.cfen_temporal_apply_u8(_lib.ptr(delta), 2, h, w, _lib.ptr(G), _lib.ptr(Y), 0, W, _lib.ptr(dst), s) == -1
    torch.cuda.synchronize()
    assert bool((dst == 9).all()) and bool((Y == 1).all())


# ---- dehaze_video.py --temporal ------------------------------------------------------------------------------------------------------------------------
CLIPS = {            # route: (frames, H, W, chroma, flags)
    "plain": (5, 128, 128, "420jpeg", []),
    "fit": (4, 150, 201, "420mpeg2", ["--fit"]),
}


def _stream(n, H, W, chroma, seed=17):
    """a y4m stream of blocky frames that change by a few levels from one to the next, and their RGB by the restatement"""
    rs = np.random.RandomState(seed)
    small = rs.randint(20, 236, ((H + 7) // 8, (W + 7) // 8, 3))
    frames = []
    for k in range(n):
        small = np.clip(small + rs.randint(-3, 4, small.shape), 0, 255)
        rgb = np.repeat(np.repeat(small.astype(np.uint8), 8, axis=0), 8, axis=1)[:H, :W]
        frames.append(yuv_ref.rgb_to_yuv(rgb, chroma, "bt601", False))
    header = yuv_ref.y4m_header(W, H, chroma)
    return yuv_ref.y4m_bytes(frames, W, H, chroma, header=header), header, [yuv_ref.yuv_to_rgb(f, H, W, chroma, "bt601", False) for f in frames]


@pytest.mark.parametrize("route", list(CLIPS))
def test_cli_temporal(route, tmp_path):
    """dehaze_video.py --temporal in child processes: the stream is, bit for bit, library route -> Stabiliser.step -> the restatement's RGB -> YCbCr,
    the same for --batchSize 1 and 2; without --temporal it is the library route alone, as before"""
    import test_hip_video as vid
    n, H, W, chroma, flags = CLIPS[route]
    vid._setup(tmp_path)
    data, header, rgb = _stream(n, H, W, chroma)
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
    st = temporal.Stabiliser()
    stab = torch.cat([st.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
    assert torch.equal(stab[0], y[0]) and not torch.equal(stab[1:], y[1:])
    changed = (stab != y).float().mean().item()
    print("%s: the stabiliser changes %.1f %% of the bytes" % (route, 100 * changed))

    def check(out_bytes, want):
        got_header, got = yuv_ref.y4m_frames(out_bytes, H, W, chroma)
        assert got_header == header and len(got) == n
        for k in range(n):
            assert np.array_equal(got[k], yuv_ref.rgb_to_yuv(want[k], chroma, "bt601", False)), (route, k)

    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "out2.y4m", flags + ["--batchSize", "2", "--temporal"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    text = r.stdout.decode()
    assert "temporal: True" in text and "temporal_strength: 0.8" in text and "video: temporal stabilisation at %d x %d (1/1)" % (W, H) in text
    check((tmp_path / "out2.y4m").read_bytes(), stab.cpu().numpy())
    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "out1.y4m", flags + ["--batchSize", "1", "--temporal"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert (tmp_path / "out1.y4m").read_bytes() == (tmp_path / "out2.y4m").read_bytes()
    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "out0.y4m", flags + ["--batchSize", "2"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "\ntemporal" not in r.stdout.decode() and "video: temporal" not in r.stdout.decode()
    check((tmp_path / "out0.y4m").read_bytes(), y.cpu().numpy())
    if route == "plain":                                       # a refusal leaves with 2 and writes nothing
        r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "none.y4m", ["--temporal_strength", "0.5"])
        assert r.returncode == 2 and b"--temporal" in r.stderr and not os.path.exists(tmp_path / "none.y4m")
        r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "none.y4m", ["--temporal", "--temporal_motion", "0"])
        assert r.returncode == 2 and b"--temporal_motion" in r.stderr and not os.path.exists(tmp_path / "none.y4m")


def test_cli_temporal_tile_route_and_noref(tmp_path):
    """the tile route with the lone first frame of an uninitialised checkpoint, and --eval_noref: the rows score the bytes that leave"""
    import test_hip_video as vid
    import test_hip_metrics as evalref
    from cfen_vit_dehazing_amd import metrics
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    from cfen_vit_dehazing_amd.manifest import generate_state_dict
    n, H, W, chroma = 3, 150, 201, "444"
    data, header, rgb = _stream(n, H, W, chroma)
    sd = generate_state_dict(evalref.TINY, seed=0, mode="reference_init")
    os.makedirs(tmp_path / "ckpt" / vid.NAME)
    torch.save(sd, tmp_path / "ckpt" / vid.NAME / "32_net_G.pth")
    (tmp_path / "in.y4m").write_bytes(data)
    r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "out.y4m", ["--tile", "--tile_overlap", "16", "--temporal", "--eval_noref"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    net = dec_ipt(evalref.TINY, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    x = dev(np.stack(rgb))
    with torch.no_grad():
        first = net.forward_tiled(x[:1], overlap=16, tile_batch=8, output_u8=True)[2]
        rest = net.forward_tiled_many([x[1], x[2]], overlap=16, tile_batch=8, output_u8=True)
    y = torch.cat([first, torch.stack([o[2] for o in rest])]).contiguous()
    stab = temporal.Stabiliser().step(x, y)
    assert not torch.equal(stab, y)
    _, got = yuv_ref.y4m_frames((tmp_path / "out.y4m").read_bytes(), H, W, chroma)
    for k in range(n):
        assert np.array_equal(got[k], yuv_ref.rgb_to_yuv(stab[k].cpu().numpy(), chroma, "bt601", False)), k
    lines = (tmp_path / "noref.csv").read_text().splitlines()
    rows = metrics.noref(x, stab, 7)
    for k, line in enumerate(lines[1:]):
        values = np.array([float(v) for v in line.split(",")[1:]])
        assert np.abs(values - np.array([float(v) for v in rows[k]])).max() <= 1e-6, k
