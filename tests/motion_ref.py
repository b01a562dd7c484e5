"""The definition of include/cfen_motion.h in numpy: what csrc/k_motion.hip and temporal.Stabiliser(mc_range > 0) compute (block matching against
the previous frame, the warp of the recursion's state, and the compensated recursion composed with tests/temporal_ref.py), and the cases and
inputs that tests/test_motion_host.py and tests/test_hip_motion.py share.

The search and the warp are integer and pure gathers: there is exactly one right answer and no tolerance.  The compensated recursion is
temporal_ref's blend and apply, unchanged, on warped inputs; its float64 form is the reference and carries temporal_ref's tolerance."""
import functools

import numpy as np

import guided_ref
import resample_ref
import temporal_ref

BLOCKS = (8, 16, 32)


def grid(h, w, block):
    """bh, bw and n_b (bh, bw): the pixels of every block, partial at the lower and right edges"""
    bh, bw = -(-h // block), -(-w // block)
    ny = np.minimum(block, h - block * np.arange(bh))
    nx = np.minimum(block, w - block * np.arange(bw))
    return bh, bw, ny[:, None] * nx[None, :]


# ---- search ---------------------------------------------------------------------------------------------------------------------------------------
def search_one(cur, prv, block, R, bias):
    """cur, prv (h, w, 3) uint8 -> vec (bh, bw, 2) int16 and sad (bh, bw) int32: every candidate in ascending (dy, dx), a candidate replaces the
    best so far only where (cost, |dy| + |dx|) is strictly smaller, so among equals the lexicographically smallest (dy, dx) stays"""
    h, w = cur.shape[:2]
    bh, bw, nb = grid(h, w, block)
    ys, xs = np.arange(bh) * block, np.arange(bw) * block
    c = cur.astype(np.int64)
    pad = np.pad(prv.astype(np.int64), ((R, R), (R, R), (0, 0)), mode="edge")                 # pad[y + R + dy] = prv[clamp(y + dy)]
    best_cost = np.full((bh, bw), np.iinfo(np.int64).max)
    best_l1 = np.zeros((bh, bw), np.int64)
    best_sad = np.zeros((bh, bw), np.int64)
    vec = np.zeros((bh, bw, 2), np.int16)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            d = np.abs(c - pad[R + dy:R + dy + h, R + dx:R + dx + w]).sum(axis=2)
            sad = np.add.reduceat(np.add.reduceat(d, ys, axis=0), xs, axis=1)
            l1 = abs(dy) + abs(dx)
            cost = 16 * sad + bias * l1 * 3 * nb
            better = (cost < best_cost) | ((cost == best_cost) & (l1 < best_l1))
            best_cost, best_l1, best_sad = np.where(better, cost, best_cost), np.where(better, l1, best_l1), np.where(better, sad, best_sad)
            vec[better] = (dy, dx)
    assert best_sad.max() < 1 << 20 and best_cost.max() < 1 << 26
    return vec, best_sad.astype(np.int32)


def search(guide, prev_guide, block, R, bias):
    """guide (B, h, w, 3), prev_guide (h, w, 3) uint8 -> vec (B, bh, bw, 2) int16, sad (B, bh, bw) int32; the predecessor of frame k is frame
    k - 1 of the call, of frame 0 it is prev_guide"""
    res = [search_one(guide[k], guide[k - 1] if k else prev_guide, block, R, bias) for k in range(len(guide))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def search_plain(cur, prv, block, R, bias):
    """the same by loops over blocks, candidates and pixels, with the lexicographic order written as a tuple comparison"""
    h, w = cur.shape[:2]
    bh, bw, _ = grid(h, w, block)
    vec, sads = np.zeros((bh, bw, 2), np.int16), np.zeros((bh, bw), np.int32)
    for by in range(bh):
        for bx in range(bw):
            pixels = [(y, x) for y in range(by * block, min(by * block + block, h)) for x in range(bx * block, min(bx * block + block, w))]
            best = None
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    sad = 0
                    for y, x in pixels:
                        q = prv[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]
                        sad += int(np.abs(cur[y, x].astype(np.int64) - q.astype(np.int64)).sum())
                    key = (16 * sad + bias * (abs(dy) + abs(dx)) * 3 * len(pixels), abs(dy) + abs(dx), dy, dx, sad)
                    best = key if best is None or key < best else best
            vec[by, bx], sads[by, bx] = (best[2], best[3]), best[4]
    return vec, sads


# ---- warp -----------------------------------------------------------------------------------------------------------------------------------------
def warp(vec, prev_guide, state, block):
    """vec (bh, bw, 2), prev_guide (h, w, 3), state (h, w, 6) -> both fetched at clamp(p + v_b)"""
    h, w = prev_guide.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    v = vec.astype(np.int64)[y // block, x // block]
    sy, sx = np.clip(y + v[..., 0], 0, h - 1), np.clip(x + v[..., 1], 0, w - 1)
    return prev_guide[sy, sx], state[sy, sx]


# ---- the compensated recursion ---------------------------------------------------------------------------------------------------------------------
class Stabiliser:
    """temporal.Stabiliser(mc_range=...) on the host, one frame at a time: step(G, Y) -> (dst bytes, v, delta, keep, vec).  mc_range = 0 is
    temporal_ref.Stabiliser; field(I, I_prev) -> vec, when given, replaces the search (for the test of the zero field)"""

    def __init__(self, radius=2, eps=1e-4, strength=0.8, motion=8.0, down="auto", dtype=np.float64, mc_range=0, mc_block=16, mc_bias=0, field=None):
        self.radius, self.eps, self.strength, self.motion, self.down, self.dtype = radius, eps, strength, motion, down, dtype
        self.mc_range, self.mc_block, self.mc_bias, self.field = mc_range, mc_block, mc_bias, field
        self.state = self.prev = None

    def step(self, G, Y):
        H, W = G.shape[:2]
        S, h, w = temporal_ref.working_size(H, W, self.down)
        I, P = (G, Y) if S == 1 else (resample_ref.pil_resize(G, (h, w), "box"), resample_ref.pil_resize(Y, (h, w), "box"))
        a, b = guided_ref.smoothed(I, P, self.radius, self.eps, self.dtype)
        coef = np.concatenate([a, b], axis=2).astype(np.float32)                           # the device stores c_t as fp32
        prev, state, vec = self.prev, self.state, None
        if state is not None and (self.mc_range or self.field):
            vec = self.field(I, prev) if self.field else search_one(I, prev, self.mc_block, self.mc_range, self.mc_bias)[0]
            prev, state = warp(vec, prev, state, self.mc_block)                            # a gather: the state stays in `dtype`, as temporal_ref's
        delta, self.state, keep, _ = temporal_ref.blend(I[None], prev, coef[None], self.radius, self.motion, self.strength, state, self.dtype)
        self.prev = I
        v = temporal_ref.apply_v(delta[0], G, Y, self.dtype)
        return temporal_ref.to_bytes(v), v, delta[0], keep[0], vec


def stabilise(G, Y, **kw):
    """the stabilised frames (n, H, W, 3) uint8 of a clip and the pre-rounding values v"""
    st = Stabiliser(**kw)
    res = [st.step(G[k], Y[k]) for k in range(len(G))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the cases of tests/test_hip_motion.py, and their inputs ----------------------------------------------------------------------------------------
SIZES = ((1, 1), (5, 7), (17, 33), (40, 50))          # one pixel; smaller than any block; partial edge blocks in both directions; several blocks
RANGES = (1, 3, 16)
KINDS = ("random", "shift", "flat", "border")


def _seed(*key):
    return sum((i + 1) * int(v) for i, v in enumerate(key)) * 37 % 100000


def frames(kind, h, w, n, seed):
    """n + 1 consecutive frames (n + 1, h, w, 3) uint8, frame 0 the predecessor.  random: independent bytes.  shift: a random texture that moves by
    a new vector within +-3 per frame (rolled, so the border wraps and matches nothing), plus noise of +-2 levels.  flat: one colour per frame,
    so every candidate of a block ties in SAD.  border: a texture that leaves the frame by 5 pixels per frame -- the best match of the blocks at
    the trailing edge lies across the clamped border"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randint(0, 256, (n + 1, h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rs.randint(0, 256, (n + 1, 1, 1, 3), dtype=np.uint8), (n + 1, h, w, 3)).copy()
    base = rs.randint(0, 256, (h + 16 * (n + 1), w + 16 * (n + 1), 3), dtype=np.uint8)
    out = []
    oy = ox = 8 * (n + 1)
    for k in range(n + 1):
        f = base[oy:oy + h, ox:ox + w].astype(np.int64)
        if kind == "shift":
            f = np.clip(f + rs.randint(-2, 3, f.shape), 0, 255)
            oy, ox = oy + rs.randint(-3, 4), ox + rs.randint(-3, 4)
        else:
            f = f.copy()
            f[:, : max(w // 3, 1)] = 200                                                     # a flat band at the left edge: the clamp repeats it
            ox += 5
        out.append(f.astype(np.uint8))
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def search_case(kind, h, w, block, R, bias, B):
    """guide (B,h,w,3), prev (h,w,3), vec (B,bh,bw,2) int16, sad (B,bh,bw) int32; computed once, read-only"""
    f = frames(kind, h, w, B, _seed(KINDS.index(kind), h, w, block, R, bias, B))
    vec, sad = search(f[1:], f[0], block, R, bias)
    out = (f[1:], f[0], vec, sad)
    for t in out:
        t.setflags(write=False)
    return out


# ---- the synthetic panning stream of the DESIGN section on motion compensation -------------------------------------------------------------------
def panning_stream(H, W, n, seed, step=(1, 3), sigma_A=4.0, sigma_t=0.03, sky=0.0, noise=0.0):
    """n frames of a camera panning over the static scattering-model scene of DESIGN section 14 (guided_ref.scattering_scene, wider and taller than
    the frame): the window moves by step = (dy, dx) pixels per frame.  The 'network' is temporal_ref.jitter_stream's: the ideal dehazer whose
    guess of the airlight jitters by N(0, sigma_A) levels per channel and of the transmission by a factor 1 + N(0, sigma_t), per frame,
    independently.  sky: that upper part of the scene is a textureless gradient (nothing there tells a block where it came from); noise: standard
    deviation, in levels, of sensor noise added to every hazy frame independently (so that no match is exact).  Returns G hazy, Y 'network' output, J clean (n, H, W, 3) uint8, and the window origins (n, 2)"""
    rs = np.random.RandomState(seed)
    sy, sx = abs(step[0]) * (n - 1), abs(step[1]) * (n - 1)
    HH, WW = H + sy, W + sx
    J0, _ = guided_ref.scattering_scene(HH, WW, seed)
    y, x = np.mgrid[0:HH, 0:WW].astype(np.float64)
    rows = int(round(sky * HH))
    J0[:rows] = (150 + 60 * y[:rows] / HH + 20 * x[:rows] / WW)[:, :, None] + np.array([-20.0, 0.0, 30.0])
    t0 = np.clip(0.6 + 0.25 * np.sin(x / WW * 3.1 + 0.5) * np.cos(y / HH * 2.3), 0.35, 0.85)[:, :, None]
    A = np.array([235.0, 240.0, 245.0])
    hazy0 = J0 * t0 + A * (1 - t0)
    G, Y, J, origin = [], [], [], []
    for k in range(n):
        oy = step[0] * k if step[0] >= 0 else sy + step[0] * k
        ox = step[1] * k if step[1] >= 0 else sx + step[1] * k
        win = (slice(oy, oy + H), slice(ox, ox + W))
        Gk, tk = temporal_ref.to_bytes(hazy0[win] + (rs.normal(0, noise, (H, W, 3)) if noise else 0.0)), t0[win]
        Ag, tg = A + rs.normal(0, sigma_A, 3), tk * (1 + rs.normal(0, sigma_t))
        G.append(Gk)
        Y.append(temporal_ref.to_bytes((Gk.astype(np.float64) - Ag * (1 - tg)) / tg))
        J.append(temporal_ref.to_bytes(J0[win]))
        origin.append((oy, ox))
    return np.stack(G), np.stack(Y), np.stack(J), np.array(origin)


def flicker_along_motion(frames_u8, origin, first=4):
    """mean |F_t(p) - F_{t-1}(p + v)| over the overlap of consecutive frames, v = origin_t - origin_{t-1} (the scene point under p in frame t lay
    under p + v in frame t - 1), over the frames `first` onward, in levels; zero for the clean scene"""
    f = frames_u8.astype(np.float64)
    H, W = f.shape[1:3]
    total, count = 0.0, 0
    for k in range(first, len(f)):
        dy, dx = (int(v) for v in origin[k] - origin[k - 1])
        cur = f[k, max(-dy, 0):H - max(dy, 0), max(-dx, 0):W - max(dx, 0)]
        old = f[k - 1, max(dy, 0):H - max(-dy, 0), max(dx, 0):W - max(-dx, 0)]
        total += np.abs(cur - old).sum()
        count += cur.size
    return total / count


psnr = guided_ref.psnr

PAN_SCENE = (96, 128, 12, 3)         # H, W, frames, seed: the scene of test_temporal_host.SCENE, panned
PAN_JITTER = (6.0, 0.04)             # as test_temporal_host.JITTER
PAN_STEP = (1, 3)                    # working-resolution pixels per frame, (dy, dx)
PAN_RANGE = 4


@functools.lru_cache(maxsize=None)
def panning_case(block, bias, sky=0.0, noise=0.0):
    """the clip of the experiment and its three runs: G, Y, J, origin, the frames of the uncompensated and of the compensated restatement;
    computed once, read-only"""
    H, W, n, seed = PAN_SCENE
    G, Y, J, origin = panning_stream(H, W, n, seed, PAN_STEP, *PAN_JITTER, sky=sky, noise=noise)
    alone, _ = stabilise(G, Y)
    mc, _ = stabilise(G, Y, mc_range=PAN_RANGE, mc_block=block, mc_bias=bias)
    out = (G, Y, J, origin, alone, mc)
    for t in out:
        t.setflags(write=False)
    return out
