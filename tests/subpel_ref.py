"""The definition of include/cfen_subpel.h in numpy, on top of tests/motion_ref.py and tests/temporal_ref.py: what csrc/k_subpel.hip and
temporal.Stabiliser(mc_subpel > 1) compute (the quarter-pixel sample of a frame, the exhaustive refinement of the whole-pixel block vectors,
the bilinear warp of the previous frame and of the recursion's state, and the compensated recursion with them), and the cases and inputs
that tests/test_subpel_host.py and tests/test_hip_subpel.py share.

The sample, the refinement and prev_out are integer: one right answer, no tolerance.  The warped state is a lerp in the dtype of the run;
float64 is the reference."""
import functools

import numpy as np

import guided_ref
import motion_ref
import resample_ref
import temporal_ref

SUBPELS = (2, 4)
VMAX = 2048                      # a whole-pixel vector is read clamped to +-VMAX, so that 4 v + 3 fits int16

grid = motion_ref.grid


# ---- the sample -------------------------------------------------------------------------------------------------------------------------------------
def taps(y4, x4, h, w):
    """the four clamped tap coordinates and the two fractions (in quarters) of the quarter-pixel positions (y4, x4), integer arrays"""
    y4, x4 = np.asarray(y4, np.int64), np.asarray(x4, np.int64)
    y0, x0 = y4 >> 2, x4 >> 2
    return (np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1), np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1), y4 & 3, x4 & 3)


def sample(img, y4, x4):
    """S(y4, x4, c) of img (h, w, C) uint8 -> int64 of shape y4.shape + (C,), in 0 .. 255"""
    h, w = img.shape[:2]
    ya, yb, xa, xb, fy, fx = taps(y4, x4, h, w)
    p = img.astype(np.int64)
    fy, fx = fy[..., None], fx[..., None]
    return ((4 - fy) * (4 - fx) * p[ya, xa] + (4 - fy) * fx * p[ya, xb] + fy * (4 - fx) * p[yb, xa] + fy * fx * p[yb, xb] + 8) >> 4


# ---- refinement -------------------------------------------------------------------------------------------------------------------------------------
def candidates(Q):
    """the offsets (ey, ex) * (4 / Q) in quarter pixels, ascending"""
    s = 4 // Q
    return [(ey * s, ex * s) for ey in range(-(Q - 1), Q) for ex in range(-(Q - 1), Q)]


def refine_one(cur, prv, vec, block, Q, bias):
    """cur, prv (h, w, 3) uint8, vec (bh, bw, 2) int16 whole pixels -> vec4 (bh, bw, 2) int16 quarter pixels and sad4 (bh, bw) int32.  The candidates
    come in ascending (dy4, dx4); one replaces the best so far only where (cost4, |dy4| + |dx4|) is strictly smaller"""
    h, w = cur.shape[:2]
    bh, bw, nb = grid(h, w, block)
    ys, xs = np.arange(bh) * block, np.arange(bw) * block
    y, x = np.mgrid[0:h, 0:w]
    c = cur.astype(np.int64)
    v0 = 4 * np.clip(vec.astype(np.int64), -VMAX, VMAX)
    best_cost = np.full((bh, bw), np.iinfo(np.int64).max)
    best_l1, best_sad = np.zeros((bh, bw), np.int64), np.zeros((bh, bw), np.int64)
    vec4 = np.zeros((bh, bw, 2), np.int16)
    for ey, ex in candidates(Q):
        v4 = v0 + np.array([ey, ex])
        vp = v4[y // block, x // block]
        d = np.abs(c - sample(prv, 4 * y + vp[..., 0], 4 * x + vp[..., 1])).sum(axis=2)
        sad = np.add.reduceat(np.add.reduceat(d, ys, axis=0), xs, axis=1)
        l1 = np.abs(v4).sum(axis=2)
        cost = 64 * sad + bias * l1 * 3 * nb
        better = (cost < best_cost) | ((cost == best_cost) & (l1 < best_l1))
        best_cost, best_l1, best_sad = np.where(better, cost, best_cost), np.where(better, l1, best_l1), np.where(better, sad, best_sad)
        vec4[better] = v4[better]
    assert best_sad.max() < 1 << 20
    return vec4, best_sad.astype(np.int32)


def refine(guide, prev_guide, vec, block, Q, bias):
    """guide (B, h, w, 3), prev_guide (h, w, 3), vec (B, bh, bw, 2) -> vec4 (B, bh, bw, 2) int16, sad4 (B, bh, bw) int32; the predecessor of frame
    k is frame k - 1 of the call, of frame 0 it is prev_guide"""
    res = [refine_one(guide[k], guide[k - 1] if k else prev_guide, vec[k], block, Q, bias) for k in range(len(guide))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def refine_plain(cur, prv, vec, block, Q, bias):
    """the same by loops over blocks, candidates and pixels, with the lexicographic order written as a tuple comparison"""
    h, w = cur.shape[:2]
    bh, bw, _ = grid(h, w, block)
    cl = lambda v, n: min(max(v, 0), n - 1)
    vec4, sads = np.zeros((bh, bw, 2), np.int16), np.zeros((bh, bw), np.int32)
    for by in range(bh):
        for bx in range(bw):
            pixels = [(y, x) for y in range(by * block, min(by * block + block, h)) for x in range(bx * block, min(bx * block + block, w))]
            dy0, dx0 = (min(max(int(v), -VMAX), VMAX) for v in vec[by, bx])
            best = None
            for ey, ex in candidates(Q):
                dy4, dx4 = 4 * dy0 + ey, 4 * dx0 + ex
                sad = 0
                for y, x in pixels:
                    y4, x4 = 4 * y + dy4, 4 * x + dx4
                    y0, x0, fy, fx = y4 >> 2, x4 >> 2, y4 & 3, x4 & 3
                    for ch in range(3):
                        p00, p01 = int(prv[cl(y0, h), cl(x0, w), ch]), int(prv[cl(y0, h), cl(x0 + 1, w), ch])
                        p10, p11 = int(prv[cl(y0 + 1, h), cl(x0, w), ch]), int(prv[cl(y0 + 1, h), cl(x0 + 1, w), ch])
                        s = ((4 - fy) * (4 - fx) * p00 + (4 - fy) * fx * p01 + fy * (4 - fx) * p10 + fy * fx * p11 + 8) >> 4
                        sad += abs(int(cur[y, x, ch]) - s)
                l1 = abs(dy4) + abs(dx4)
                key = (64 * sad + bias * l1 * 3 * len(pixels), l1, dy4, dx4, sad)
                best = key if best is None or key < best else best
            vec4[by, bx], sads[by, bx] = (best[2], best[3]), best[4]
    return vec4, sads


# ---- warp -------------------------------------------------------------------------------------------------------------------------------------------
def warp(vec4, prev_guide, state, block, dtype=np.float64):
    """vec4 (bh, bw, 2) quarter pixels, prev_guide (h, w, 3) uint8, state (h, w, 6) -> prev_out (h, w, 3) uint8 = S(4 p + v4_b) and state_out
    (h, w, 6) in `dtype`: t0 = s00 + fx (s01 - s00), t1 = s10 + fx (s11 - s10), t0 + fy (t1 - t0)"""
    h, w = prev_guide.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    v = vec4.astype(np.int64)[y // block, x // block]
    y4, x4 = 4 * y + v[..., 0], 4 * x + v[..., 1]
    ya, yb, xa, xb, fy, fx = taps(y4, x4, h, w)
    s = state.astype(dtype)
    fy, fx = (fy.astype(dtype) / dtype(4))[..., None], (fx.astype(dtype) / dtype(4))[..., None]
    t0 = s[ya, xa] + fx * (s[ya, xb] - s[ya, xa])
    t1 = s[yb, xa] + fx * (s[yb, xb] - s[yb, xa])
    out = t0 + fy * (t1 - t0)
    assert out.dtype == dtype
    return sample(prev_guide, y4, x4).astype(np.uint8), out


def tap_magnitude(vec4, state, block):
    """M (h, w, 6): the largest magnitude among the four taps of every output, for the bound of the device's warped state"""
    h, w = state.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    v = vec4.astype(np.int64)[y // block, x // block]
    ya, yb, xa, xb, _, _ = taps(4 * y + v[..., 0], 4 * x + v[..., 1], h, w)
    a = np.abs(state.astype(np.float64))
    return np.maximum(np.maximum(a[ya, xa], a[ya, xb]), np.maximum(a[yb, xa], a[yb, xb]))


# ---- the compensated recursion ----------------------------------------------------------------------------------------------------------------------
class Stabiliser:
    """temporal.Stabiliser(mc_range=..., mc_subpel=...) on the host, one frame at a time: step(G, Y) -> (dst bytes, v, delta, keep, vec4).
    mc_subpel = 1 is motion_ref.Stabiliser (vec4 is then its whole-pixel vec)"""

    def __init__(self, radius=2, eps=1e-4, strength=0.8, motion=8.0, down="auto", dtype=np.float64, mc_range=0, mc_block=16, mc_bias=0, mc_subpel=1):
        self.radius, self.eps, self.strength, self.motion, self.down, self.dtype = radius, eps, strength, motion, down, dtype
        self.mc_range, self.mc_block, self.mc_bias, self.mc_subpel = mc_range, mc_block, mc_bias, mc_subpel
        self.state = self.prev = None

    def step(self, G, Y):
        H, W = G.shape[:2]
        S, h, w = temporal_ref.working_size(H, W, self.down)
        I, P = (G, Y) if S == 1 else (resample_ref.pil_resize(G, (h, w), "box"), resample_ref.pil_resize(Y, (h, w), "box"))
        a, b = guided_ref.smoothed(I, P, self.radius, self.eps, self.dtype)
        coef = np.concatenate([a, b], axis=2).astype(np.float32)                           # the device stores c_t as fp32
        prev, state, vec = self.prev, self.state, None
        if state is not None and self.mc_range:
            vec = motion_ref.search_one(I, prev, self.mc_block, self.mc_range, self.mc_bias)[0]
            if self.mc_subpel > 1:
                vec = refine_one(I, prev, vec, self.mc_block, self.mc_subpel, self.mc_bias)[0]
                prev, state = warp(vec, prev, state, self.mc_block, self.dtype)
            else:
                prev, state = motion_ref.warp(vec, prev, state, self.mc_block)
        delta, self.state, keep, _ = temporal_ref.blend(I[None], prev, coef[None], self.radius, self.motion, self.strength, state, self.dtype)
        self.prev = I
        v = temporal_ref.apply_v(delta[0], G, Y, self.dtype)
        return temporal_ref.to_bytes(v), v, delta[0], keep[0], vec


def stabilise(G, Y, **kw):
    """the stabilised frames (n, H, W, 3) uint8 of a clip and the pre-rounding values v"""
    st = Stabiliser(**kw)
    res = [st.step(G[k], Y[k]) for k in range(len(G))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the cases of tests/test_hip_subpel.py, and their inputs ----------------------------------------------------------------------------------------
SIZES = motion_ref.SIZES
BLOCKS = motion_ref.BLOCKS
KINDS = ("random", "subshift", "flat", "border")
BIASES = (0, 4)


def subshift(h, w, n, Q, seed, gain=4.0):
    """n + 1 consecutive frames (n + 1, h, w, 3) uint8 of a texture that moves by a fraction of a pixel per frame: random bytes on a grid of
    quarter pixels, smoothed with a 6-tap box per axis, read at an origin that moves by (a, b) quarter pixels per frame, a and b odd multiples of
    4 / Q, box-reduced x 4, plus noise of +-1 level.  gain: the contrast given back after the smoothing (the texture of the refinement tests has
    gradients of some 30 levels per pixel, which switches the recursion off at any misalignment: the clips of the recursion's tests take gain 1)"""
    rs = np.random.RandomState(seed)
    s = 4 // Q
    m = 8 * (n + 1) + 8
    t = rs.randint(0, 256, (4 * h + 2 * m + 5, 4 * w + 2 * m + 5, 3)).astype(np.float64)
    t = sum(t[i:t.shape[0] - 5 + i] for i in range(6)) / 6
    t = sum(t[:, i:t.shape[1] - 5 + i] for i in range(6)) / 6
    t = np.clip(128 + (t - 128) * gain, 0, 255)                                            # the box took most of the contrast: give it back
    oy = ox = m
    out = []
    for k in range(n + 1):
        f = t[oy:oy + 4 * h, ox:ox + 4 * w].reshape(h, 4, w, 4, 3).mean(axis=(1, 3))
        out.append(np.clip(np.floor(f + 0.5) + rs.randint(-1, 2, f.shape), 0, 255).astype(np.uint8))
        oy, ox = oy + s * rs.choice([-3, -1, 1, 3]), ox + s * rs.choice([-3, -1, 1, 3])
    return np.stack(out)


def frames(kind, h, w, n, Q, seed):
    return subshift(h, w, n, Q, seed) if kind == "subshift" else motion_ref.frames(kind, h, w, n, seed)


def hand_vec(bh, bw, B, seed):
    """a hand-made whole-pixel field with entries at +-16, so that the taps of the blocks at the edges cross the clamped border"""
    rs = np.random.RandomState(seed)
    return rs.choice(np.array([-16, 16, 0, 3, -5], np.int16), size=(B, bh, bw, 2))


@functools.lru_cache(maxsize=None)
def refine_case(kind, h, w, block, Q, bias, B, hand=False):
    """guide (B,h,w,3), prev (h,w,3), vec (B,bh,bw,2) int16, vec4 (B,bh,bw,2) int16, sad4 (B,bh,bw) int32; computed once, read-only"""
    f = frames(kind, h, w, B, Q, motion_ref._seed(KINDS.index(kind), h, w, block, Q, bias, B))
    bh, bw, _ = grid(h, w, block)
    vec = hand_vec(bh, bw, B, h + w + block) if hand else motion_ref.search(f[1:], f[0], block, 3, bias)[0]
    vec4, sad4 = refine(f[1:], f[0], vec, block, Q, bias)
    out = (f[1:], f[0], vec, vec4, sad4)
    for t in out:
        t.setflags(write=False)
    return out


def fractional_share(vec4):
    """the share of blocks whose vector is not a whole number of pixels"""
    return float(((vec4.astype(np.int64) & 3) != 0).any(axis=-1).mean())


# ---- the experiment of the DESIGN section on sub-pixel vectors ---------------------------------------------------------------------------------------
# (H, W, step per frame at full resolution, down, sky, noise): the scene, jitter, frames and seed are motion_ref's PAN_SCENE[2:], PAN_JITTER
CLIPS = {"half": (192, 256, (1, 3), 2, 0.0, 0.0), "half_hard": (192, 256, (1, 3), 2, 0.4, 2.0), "quarter": (384, 512, (3, 5), 4, 0.0, 0.0),
         "whole": (192, 256, (2, 6), 2, 0.0, 0.0)}


@functools.lru_cache(maxsize=None)
def clip(name):
    """G, Y, J, origin of a clip of the experiment; computed once, read-only"""
    H, W, step, down, sky, noise = CLIPS[name]
    _, _, n, seed = motion_ref.PAN_SCENE
    out = motion_ref.panning_stream(H, W, n, seed, step, *motion_ref.PAN_JITTER, sky=sky, noise=noise)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def clip_run(name, Q, block=16, bias=4):
    """the frames of the restatement on a clip: Q = 0 is --temporal alone, 1 whole-pixel compensation, 2 and 4 refined; read-only"""
    G, Y, _, _ = clip(name)
    down = CLIPS[name][3]
    kw = dict(mc_range=motion_ref.PAN_RANGE, mc_block=block, mc_bias=bias, mc_subpel=Q) if Q else {}
    out, _ = stabilise(G, Y, down=down, **kw)
    out.setflags(write=False)
    return out


def clip_scores(name, frames_u8):
    """(flicker along the true motion at full resolution, PSNR against the clean frames from frame 4 on)"""
    _, _, J, origin = clip(name)
    return motion_ref.flicker_along_motion(frames_u8, origin), motion_ref.psnr(frames_u8[4:], J[4:])
