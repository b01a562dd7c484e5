"""The definition of include/cfen_temporal.h in numpy: what csrc/k_temporal.hip and cfen_vit_dehazing_amd/temporal.py compute (temporal
stabilisation of a dehazed stream), and the cases and inputs that tests/test_temporal_host.py and tests/test_hip_temporal.py share.

dtype=float64 is the reference.  dtype=float32 follows the header's formulas and order step by step with every operation rounded to fp32; it
exists only to size the tolerance (test_temporal_host.TAU_T).  The scalar parameters are the fp32 values the device is handed, in both forms.
The coefficients of step 2 and the upsampling of step 5 are those of tests/guided_ref.py, unchanged."""
import functools

import numpy as np

import guided_ref
import resample_ref


def _p(x, dtype):
    """a scalar parameter as the device receives it (fp32), in the working dtype"""
    return dtype(np.float32(x))


# ---- steps 3 and 4 -------------------------------------------------------------------------------------------------------------------------------
def motion_sum(I, Iprev, r):
    """D (h, w) int64: the window sum of sum_c |I - Iprev|, exact"""
    d = np.abs(I.astype(np.int64) - Iprev.astype(np.int64)).sum(axis=2)
    return guided_ref.box_sum(d, r)


def keep_of(D, N, motion, dtype=np.float64):
    d = D.astype(dtype) / (3 * N).astype(dtype)
    keep = np.clip(dtype(1) - d / _p(motion, dtype), dtype(0), dtype(1))
    assert keep.dtype == dtype
    return keep


def blend(guide, prev_guide, coef, r, motion, strength, state=None, dtype=np.float64):
    """guide (B, h, w, 3) uint8, prev_guide (h, w, 3) uint8 or None, coef (B, h, w, 6) fp32, state (h, w, 6) or None (the first frame of a stream)
    -> delta (B, h, w, 6), state (h, w, 6), keep (B, h, w) in `dtype` (keep of a stream's first frame is 0 by convention), D (B, h, w) int64
    (-1 for a stream's first frame)"""
    B, h, w, _ = guide.shape
    N = guided_ref.window_count(h, w, r)
    S = None if state is None else state.astype(dtype)
    deltas, keeps, Ds = [], [], []
    for k in range(B):
        c = coef[k].astype(dtype)
        if S is None:
            S, keep, D = c, np.zeros((h, w), dtype), np.full((h, w), -1, np.int64)
        else:
            D = motion_sum(guide[k], guide[k - 1] if k else prev_guide, r)
            keep = keep_of(D, N, motion, dtype)
            kk = (_p(strength, dtype) * keep)[:, :, None]
            S = c + kk * (S - c)
        assert S.dtype == dtype
        deltas.append(S - c)
        keeps.append(keep)
        Ds.append(D)
    return np.stack(deltas), S, np.stack(keeps), np.stack(Ds)


# ---- step 5 ---------------------------------------------------------------------------------------------------------------------------------------
def apply_v(delta, G, Y, dtype=np.float64):
    """the pre-rounding value v (H, W, 3) of one frame: delta (h, w, 6), G and Y (H, W, 3) uint8"""
    H, W = G.shape[:2]
    up = guided_ref.upsample(delta.astype(dtype), H, W, dtype)
    v = (Y.astype(dtype) + up[..., :3] * G.astype(dtype)) + up[..., 3:]
    assert v.dtype == dtype
    return v


to_bytes = guided_ref.to_bytes


# ---- the whole pipeline ------------------------------------------------------------------------------------------------------------------------------
def working_size(H, W, down="auto"):
    S = -(-max(H, W) // 1024) if down == "auto" else int(down)
    return S, -(-H // S), -(-W // S)


class Stabiliser:
    """cfen_vit_dehazing_amd.temporal.Stabiliser on the host, one frame at a time: step(G, Y) -> (dst bytes, v, delta, keep)"""

    def __init__(self, radius=2, eps=1e-4, strength=0.8, motion=8.0, down="auto", dtype=np.float64):
        self.radius, self.eps, self.strength, self.motion, self.down, self.dtype = radius, eps, strength, motion, down, dtype
        self.reset()

    def reset(self):
        self.state = self.prev = None

    def step(self, G, Y):
        H, W = G.shape[:2]
        S, h, w = working_size(H, W, self.down)
        I, P = (G, Y) if S == 1 else (resample_ref.pil_resize(G, (h, w), "box"), resample_ref.pil_resize(Y, (h, w), "box"))
        a, b = guided_ref.smoothed(I, P, self.radius, self.eps, self.dtype)
        coef = np.concatenate([a, b], axis=2).astype(np.float32)                           # the device stores c_t as fp32
        delta, self.state, keep, _ = blend(I[None], self.prev, coef[None], self.radius, self.motion, self.strength, self.state, self.dtype)
        self.prev = I
        v = apply_v(delta[0], G, Y, self.dtype)
        return to_bytes(v), v, delta[0], keep[0]


# ---- the cases of tests/test_hip_temporal.py, and their inputs --------------------------------------------------------------------------------------
SIZES = ((1, 1), (3, 5), (17, 33), (40, 50))          # one pixel; smaller than a tile; 2 x 3 tiles with one-pixel remainders; 3 x 4 tiles
RADII = (1, 2, 16)
BATCHES = (1, 3, 4)
MOTION, STRENGTH = 8.0, 0.8
TRANSITIONS = ("same", "noise", "cut", "patch")


def frames(h, w, n, seed):
    """n + 1 consecutive frames (n + 1, h, w, 3) uint8: frame 0 is the predecessor; transition k is TRANSITIONS[(seed + k) % 4] -- an identical
    frame, +-2 levels on a third of the bytes, a new random frame, or a new random block in an unchanged frame"""
    rs = np.random.RandomState(seed)
    out = [rs.randint(0, 256, (h, w, 3), dtype=np.uint8)]
    for k in range(n):
        kind = TRANSITIONS[(seed + k) % 4]
        f = out[-1].copy()
        if kind == "noise":
            f = np.clip(f.astype(np.int64) + rs.randint(-2, 3, f.shape) * (rs.rand(*f.shape) < 0.33), 0, 255).astype(np.uint8)
        elif kind == "cut":
            f = (f.astype(np.int64) + rs.randint(64, 192, f.shape)).astype(np.uint8)         # every byte changes by at least 64 levels (mod 256)
        elif kind == "patch":
            y0, x0 = rs.randint(0, h), rs.randint(0, w)
            f[y0:y0 + max(h // 3, 1), x0:x0 + max(w // 3, 1)] = rs.randint(0, 256, f[y0:y0 + max(h // 3, 1), x0:x0 + max(w // 3, 1)].shape, dtype=np.uint8)
        out.append(f)
    return np.stack(out)


def coefficients(n, h, w, seed):
    """(n, h, w, 6) fp32, given, not fitted: slopes within +-2 and offsets within +-300 levels, what the fit of 8-bit frames spans"""
    rs = np.random.RandomState(seed + 7)
    return np.concatenate([rs.uniform(-2, 2, (n, h, w, 3)), rs.uniform(-300, 300, (n, h, w, 3))], axis=3).astype(np.float32)


def _seed(*key):
    return sum((i + 1) * int(v) for i, v in enumerate(key)) * 31 % 100000


@functools.lru_cache(maxsize=None)
def blend_case(h, w, r, B, have_state):
    """guide (B,h,w,3), prev (h,w,3), coef (B,h,w,6), state0 (h,w,6) fp32 or None, and the float64 delta, state, keep, D; computed once, read-only"""
    seed = _seed(h, w, r, B, have_state)
    f = frames(h, w, B, seed)
    coef = coefficients(B, h, w, seed)
    state0 = coefficients(1, h, w, seed + 1)[0] if have_state else None
    delta, state, keep, D = blend(f[1:], f[0] if have_state else None, coef, r, MOTION, STRENGTH, state0)
    out = (f[1:], f[0], coef, state0, delta, state, keep, D)
    for t in out:
        if t is not None:
            t.setflags(write=False)
    return out


# (h, w) -> (H, W): the smallest shapes that reach each path of k_temporal_apply (4096 bytes of one output row per workgroup, a lane 16)
APPLY_CASES = {
    "17x33_1to1": ((17, 33), (17, 33)),                     # 99-byte rows, byte path; the working resolution IS the frame: fy = fx = 0
    "40x32_1to1": ((40, 32), (40, 32)),                     # 96-byte rows: 3 W is a multiple of 16, the vector path
    "13x21_37x61": ((13, 21), (37, 61)),                    # upsampling, 183-byte rows
    "3x350_2x1400": ((3, 350), (2, 1400)),                  # 4200-byte rows: two workgroups per row, 343 columns staged in LDS; byte path
    "3x344_2x1376": ((3, 344), (2, 1376)),                  # the same on the vector path (4128-byte rows)
    "2x1400_1to1": ((2, 1400), (2, 1400)),                  # 1:1 and wide: the first workgroup covers 1367 columns, the global-memory path
    "2x1376_1to1": ((2, 1376), (2, 1376)),                  # the same on the vector path
}


@functools.lru_cache(maxsize=None)
def apply_case(name):
    """delta (1,h,w,6) fp32 (given: a tenth of the coefficients' span, and zero on a block so that some bytes must pass unchanged), G, Y
    (1,H,W,3) uint8 and the float64 pre-rounding v (1,H,W,3); computed once, read-only"""
    (h, w), (H, W) = APPLY_CASES[name]
    seed = _seed(h, w, H, W)
    rs = np.random.RandomState(seed)
    delta = coefficients(1, h, w, seed) * np.float32(0.1)
    delta[:, : (h + 1) // 2, : (w + 1) // 2] = 0
    G, Y = rs.randint(0, 256, (1, H, W, 3), dtype=np.uint8), rs.randint(0, 256, (1, H, W, 3), dtype=np.uint8)
    out = (delta, G, Y, apply_v(delta[0], G[0], Y[0])[None])
    for t in out:
        t.setflags(write=False)
    return out


# ---- the synthetic stream of DESIGN section 18 ---------------------------------------------------------------------------------------------------
def jitter_stream(H, W, n, seed, sigma_A=4.0, sigma_t=0.03, moving=False, cut_at=None):
    """n frames of the scattering-model scene of DESIGN section 14 (guided_ref.scattering_scene), dehazed by the ideal dehazer with a wrong guess:
    per frame, independently, the airlight it assumes is A + N(0, sigma_A) levels per channel and the transmission t (1 + N(0, sigma_t)).
    moving: a textured 24 x 32 object crosses the scene, 3 pixels per frame.  cut_at: from that frame on another scene (the first one mirrored,
    dark, through thin haze).  Returns G (n,H,W,3) uint8 hazy, Y (n,H,W,3) uint8 'network' output, J (n,H,W,3) uint8 ideal, and the object's
    footprint (n,H,W) bool"""
    rs = np.random.RandomState(seed)
    J0, _ = guided_ref.scattering_scene(H, W, seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t0 = np.clip(0.6 + 0.25 * np.sin(x / W * 3.1 + 0.5) * np.cos(y / H * 2.3), 0.35, 0.85)[:, :, None]
    A = np.array([235.0, 240.0, 245.0])
    obj = np.clip(60 + 40 * np.sin(x[:24, :32, None] / 2.1) * np.cos(y[:24, :32, None] / 1.7) + np.array([40.0, -10.0, 20.0]), 0, 255)
    G, Y, J, F = [], [], [], []
    for k in range(n):
        Jk, tk = J0.copy(), t0
        if cut_at is not None and k >= cut_at:
            Jk, tk = J0[::-1, ::-1] * 0.3, np.minimum(t0 * 1.4, 0.95)                       # a dark scene through thin haze: far from the first everywhere
        foot = np.zeros((H, W), bool)
        if moving:
            oy, ox = H // 3, 4 + 3 * k
            Jk[oy:oy + 24, ox:ox + 32] = obj[:, : max(min(32, W - ox), 0)]
            foot[oy:oy + 24, ox:ox + 32] = True
        hazy = Jk * tk + A * (1 - tk)
        Gk = to_bytes(hazy)
        Ag, tg = A + rs.normal(0, sigma_A, 3), tk * (1 + rs.normal(0, sigma_t))
        G.append(Gk)
        Y.append(to_bytes((Gk.astype(np.float64) - Ag * (1 - tg)) / tg))
        J.append(to_bytes(Jk))
        F.append(foot)
    return np.stack(G), np.stack(Y), np.stack(J), np.stack(F)


def flicker(frames_u8, first=4):
    """mean |out_t - out_{t-1}| over the frames `first` onward, in levels"""
    f = frames_u8.astype(np.float64)
    return float(np.mean(np.abs(f[first:] - f[first - 1:-1])))


psnr = guided_ref.psnr
