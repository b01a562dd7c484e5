"""The definition of include/cfen_guided.h in numpy: what csrc/k_guided.hip computes (guided upsampling of uint8 RGB images), and the cases and
inputs that tests/test_guided_host.py and tests/test_hip_guided.py share.

dtype=float64 is the reference.  dtype=float32 follows the header's formulas and order step by step with every operation rounded to fp32, the
window sums as direct sums (row by row, each row from left to right); it exists only to size the tolerance (test_guided_host.TAU).  The *_brute
functions are the same definitions with explicit loops over every window, for tiny shapes."""
import functools

import numpy as np


# ---- window sums ------------------------------------------------------------------------------------------------------------------------------
def counts(n, r):
    """N along one axis: pixels of [p - r, p + r] inside [0, n)"""
    p = np.arange(n)
    return np.minimum(p + r, n - 1) - np.maximum(p - r, 0) + 1


def window_count(h, w, r):
    return counts(h, r)[:, None] * counts(w, r)[None, :]


def _box_axis(a, r, axis):
    """clipped window sums along `axis` by a cumulative sum (the dtype of `a`: exact for integers)"""
    n = a.shape[axis]
    a = np.moveaxis(a, axis, 0)
    c = np.concatenate([np.zeros((1,) + a.shape[1:], a.dtype), np.cumsum(a, axis=0, dtype=a.dtype)])
    p = np.arange(n)
    out = c[np.minimum(p + r, n - 1) + 1] - c[np.maximum(p - r, 0)]
    return np.moveaxis(out, 0, axis)


def box_sum(a, r):
    """sum over the clipped (2r+1)^2 window around every pixel of a (h, w, ...): rows, then columns"""
    return _box_axis(_box_axis(a, r, 1), r, 0)


def box_sum_brute(a, r):
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    for y in range(h):
        for x in range(w):
            acc = np.zeros(a.shape[2:], a.dtype)
            for q in range(max(y - r, 0), min(y + r, h - 1) + 1):
                for p in range(max(x - r, 0), min(x + r, w - 1) + 1):
                    acc = acc + a[q, p]
            out[y, x] = acc
    return out


def box_sum_direct(a, r):
    """the same sums in the dtype of `a`, term by term in the order the header names: the rows of a window from top to bottom ... each row summed
    from left to right first (zeros outside the image add exactly)"""
    h, w = a.shape[:2]
    pad = np.zeros((h + 2 * r, w + 2 * r) + a.shape[2:], a.dtype)
    pad[r:r + h, r:r + w] = a
    rows = np.zeros((h + 2 * r, w) + a.shape[2:], a.dtype)
    for d in range(2 * r + 1):
        rows = rows + pad[:, d:d + w]
    out = np.zeros_like(a)
    for d in range(2 * r + 1):
        out = out + rows[d:d + h]
    return out


def statistics(I, P, r, box=box_sum):
    """N (h, w) and S_I, S_P, S_II, S_IP (h, w, 3), exact in int64"""
    I, P = I.astype(np.int64), P.astype(np.int64)
    return window_count(I.shape[0], I.shape[1], r), box(I, r), box(P, r), box(I * I, r), box(I * P, r)


# ---- coefficients -----------------------------------------------------------------------------------------------------------------------------
def eps255(eps, dtype):
    return dtype(np.float32(eps * 255.0 * 255.0)) if dtype is np.float32 else dtype(eps * 255.0 * 255.0)


def coefficients(I, P, r, eps, dtype=np.float64, box=box_sum):
    """a, b (h, w, 3) of one image"""
    N, SI, SP, SII, SIP = statistics(I, P, r, box)
    N = N[:, :, None]
    C = N * SIP - SI * SP
    V = N * SII - SI * SI
    f = lambda v: v.astype(dtype)                                                            # int64 -> fp32 rounds to nearest, as the device does
    a = f(C) / (f(V) + eps255(eps, dtype) * f(N * N))
    b = (f(SP) - a * f(SI)) / f(N)
    assert a.dtype == dtype and b.dtype == dtype
    return a, b


def smoothed(I, P, r, eps, dtype=np.float64, brute=False):
    """abar, bbar (h, w, 3) of one image"""
    a, b = coefficients(I, P, r, eps, dtype, box_sum_brute if brute else box_sum)
    box = box_sum_brute if brute else (box_sum_direct if dtype is np.float32 else box_sum)
    N = window_count(I.shape[0], I.shape[1], r)[:, :, None].astype(dtype)
    return box(a, r) / N, box(b, r) / N


# ---- upsampling -------------------------------------------------------------------------------------------------------------------------------
def axis_coords(n_in, n_out, dtype=np.float64):
    """i0, i1, f per output index: the exact rational ((2i+1) n_in - n_out) / (2 n_out), clamped below at 0, in integers"""
    i = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * i + 1) * n_in - n_out, 0)
    den = 2 * n_out
    i0 = num // den
    f = (num - i0 * den).astype(dtype) / dtype(den)
    return i0, np.minimum(i0 + 1, n_in - 1), f


def upsample(c, H, W, dtype=np.float64):
    """c (h, w, k) -> (H, W, k): vertically first, cv = c(y0) + fy (c(y1) - c(y0)), then horizontally"""
    c = c.astype(dtype)
    y0, y1, fy = axis_coords(c.shape[0], H, dtype)
    x0, x1, fx = axis_coords(c.shape[1], W, dtype)
    cv = c[y0] + fy[:, None, None] * (c[y1] - c[y0])
    out = cv[:, x0] + fx[None, :, None] * (cv[:, x1] - cv[:, x0])
    assert out.dtype == dtype
    return out


def guided_v(G, I, P, r, eps, dtype=np.float64):
    """the pre-rounding value v (H, W, 3) of one image"""
    abar, bbar = smoothed(I, P, r, eps, dtype)
    H, W = G.shape[:2]
    v = upsample(abar, H, W, dtype) * G.astype(dtype) + upsample(bbar, H, W, dtype)
    assert v.dtype == dtype
    return v


def to_bytes(v):
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def guided_upsample(G, I, P, r=2, eps=1e-4, dtype=np.float64):
    return to_bytes(guided_v(G, I, P, r, eps, dtype))


# ---- the cases of tests/test_hip_guided.py, and their inputs -------------------------------------------------------------------------------------
EPS = (1e-4, 1e-2)
KINDS = ("random", "model", "binary")

# (B, h, w, r): the smallest shapes that reach each path of k_guided_coef / k_guided_mean (tiles of 16 x 16 pixels with a halo of r)
COEF_CASES = {
    "1x1_r1": (1, 1, 1, 1),                   # one pixel: every window is that pixel, 255 idle threads
    "5x7_r16": (1, 5, 7, 16),                 # every window is the whole image: the halo lies outside it on all sides
    "33x40_r1": (2, 33, 40, 1),               # 3 x 3 tiles, the last row and column of tiles hold one and eight pixels; two images
    "33x40_r4": (1, 33, 40, 4),
    "17x70_r2": (3, 17, 70, 2),               # 2 x 5 tiles, three images
    "64x96_r16": (1, 64, 96, 16),             # several tiles at the largest halo: the 48 x 48 staged region, inner tiles with no clipping
    "128x128_r2": (1, 128, 128, 2),           # the tiny net's T at the default radius
}

# (h, w) -> (H, W), r, kind: the smallest shapes that reach each path of k_guided_apply (4096 bytes of one output row per workgroup, a lane 16)
APPLY_CASES = {
    "1x1_3x5": ((1, 1), (3, 5), 1, "random"),                 # one coefficient: y1 = y0, x1 = x0; 15-byte rows, byte path
    "5x7_37x53": ((5, 7), (37, 53), 2, "model"),              # 159-byte rows, byte path, the last lane owns 15 bytes
    "33x40_16x16": ((33, 40), (16, 16), 2, "model"),          # downward; 48-byte rows, vector path
    "64x96_128x200": ((64, 96), (128, 200), 2, "model"),      # 600-byte rows: byte path (600 % 16 = 8)
    "33x40_33x97": ((33, 40), (33, 97), 4, "random"),         # one axis unchanged: fy = 0 on every row
    "20x24_30x400": ((20, 24), (30, 400), 2, "model"),        # 1200-byte rows, vector path, 75 lanes = more than one wave's run per row
    "16x16_120x120": ((16, 16), (120, 120), 2, "model"),      # 7.5 x, the workload's ratio; 360-byte rows: byte path
    "8x8_1x24": ((8, 8), (1, 24), 1, "random"),
    "8x8_20x1": ((8, 8), (20, 1), 1, "random"),               # 3-byte rows
    "12x14_20x31_binary": ((12, 14), (20, 31), 1, "binary_clip"),  # 0/255 output and guide: v leaves [0, 255] at both ends, the clamp on both sides
    "6x2100_3x1400": ((6, 2100), (3, 1400), 1, "model"),      # 4200-byte rows: two workgroups per row, the second begins inside a pixel; the first
                                                              # covers 2049 coefficient columns: more than are staged, the global-memory path (byte path)
    "4x1500_2x1376": ((4, 1500), (2, 1376), 1, "random"),     # 4128-byte rows, vector path, two workgroups, the first on the global-memory path
    "40x30_3x1400": ((40, 30), (3, 1400), 2, "model"),        # 4200-byte rows upward: two workgroups per row on the staged path, byte path
    "4x30_2x1376": ((4, 30), (2, 1376), 1, "model"),          # the same on the vector path; the second workgroup owns 32 bytes
}


def lowres(kind, B, h, w, seed):
    """I, P (B, h, w, 3) uint8.  random: independent bytes; model: a smooth guide with pixel noise and P = 0.8 I + noise + 30; binary: 0 / 255"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        return rs.randint(0, 256, (B, h, w, 3), dtype=np.uint8), rs.randint(0, 256, (B, h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rs.randint(0, 2, (B, h, w, 3)) * 255).astype(np.uint8), (rs.randint(0, 2, (B, h, w, 3)) * 255).astype(np.uint8)
    if kind == "binary_clip":
        # P (and the full-resolution guide, hires) 0 / 255; I takes the two values 96 and 160 and follows P nine times in ten.  With I 0 / 255 as
        # well every window's line maps [0, 255] into [0, 255] and so does any mean of such lines: v can leave the range only where the guide
        # leaves the local range of I.  Here the line through (96, 0) and (160, 255) is near -380 at G = 0 and near 630 at G = 255
        P = rs.rand(B, h, w, 3) < 0.5
        I = P ^ (rs.rand(B, h, w, 3) < 0.1)
        return (96 + 64 * I).astype(np.uint8), (P * 255).astype(np.uint8)
    assert kind == "model", kind
    y, x = np.mgrid[0:h, 0:w]
    ph = rs.uniform(0, 6.28, (B, 1, 1, 3))
    smooth = 128 + 70 * np.sin(y[None, :, :, None] / 5.0 + ph) * np.cos(x[None, :, :, None] / 7.0 + ph)
    I = np.clip(np.round(smooth + rs.normal(0, 12, (B, h, w, 3))), 0, 255).astype(np.uint8)
    P = np.clip(np.round(0.8 * I + rs.normal(0, 3, (B, h, w, 3)) + 30), 0, 255).astype(np.uint8)
    return I, P


def hires(kind, B, H, W, seed):
    rs = np.random.RandomState(seed + 1000)
    if kind in ("binary", "binary_clip"):
        return (rs.randint(0, 2, (B, H, W, 3)) * 255).astype(np.uint8)
    return rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8)


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % 100000


@functools.lru_cache(maxsize=None)
def coef_case(name, kind, eps):
    """I, P and the float64 abar, bbar (B, h, w, 3) of a coefficient case; computed once, shared, read-only"""
    B, h, w, r = COEF_CASES[name]
    I, P = lowres(kind, B, h, w, _seed(name + kind))
    ab = [smoothed(I[i], P[i], r, eps) for i in range(B)]
    out = (I, P, np.stack([a for a, _ in ab]), np.stack([b for _, b in ab]))
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def apply_case(name):
    """G, I, P and the float64 pre-rounding v (1, H, W, 3) of an apply case at eps 1e-4; computed once, shared, read-only"""
    (h, w), (H, W), r, kind = APPLY_CASES[name]
    I, P = lowres(kind, 1, h, w, _seed(name))
    G = hires(kind, 1, H, W, _seed(name))
    out = (G, I, P, guided_v(G[0], I[0], P[0], r, 1e-4)[None])
    for t in out:
        t.setflags(write=False)
    return out


# ---- the scattering-model scene of DESIGN section 14 ----------------------------------------------------------------------------------------------
def scattering_scene(H, W, seed):
    """clear J and hazy I = J t + A (1 - t), (H, W, 3) float64 on the 0..255 scale: pixel-scale texture, smooth transmission t in 0.35 .. 0.85,
    airlight A = (235, 240, 245)"""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 120 + 45 * np.sin(x / 23.0)[:, :, None] * np.cos(y / 17.0)[:, :, None] + np.array([10.0, 0.0, -10.0])
    ph = rs.uniform(0, 6.28, 3)
    base = base + 35 * np.sin(x[:, :, None] / 2.9 + ph) * np.sin(y[:, :, None] / 3.7 - ph)    # objects a few low-resolution pixels wide
    J = np.clip(base + rs.normal(0, 12, (H, W, 3)), 0, 255)                                  # independent noise per pixel: texture at the pixel scale
    t = 0.6 + 0.25 * np.sin(x / W * 3.1 + 0.5) * np.cos(y / H * 2.3)
    t = np.clip(t, 0.35, 0.85)[:, :, None]
    A = np.array([235.0, 240.0, 245.0])
    return J, J * t + A * (1 - t)


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
