"""The no-reference statistics of include/cfen_noref.h restated in numpy: integers for everything but the gradient sum, float64 there; the scores
of metrics.noref_from_stats restated beside them; and the case list tests/test_hip_noref.py runs on the device.  Not a test module."""
import functools

import numpy as np

COLUMNS = ("dark_in", "dark_out", "entropy_in", "entropy_out", "avg_gradient_in", "avg_gradient_out", "contrast_in", "contrast_out", "saturated")
TILE_W, TILE_H = 64, 64          # the kernel's tile (CFEN_NOREF_TILE_W / _H; ops.NOREF_TILE_W / _H -- test_noref_host.py holds the three together)


def luma(img):
    """(..., 3) uint8 -> (...) int64 in 0 .. 255: (77 R + 150 G + 29 B + 128) >> 8"""
    v = np.asarray(img).astype(np.int64)
    return (77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8


def dark_channel(img, r):
    """(H, W, 3) uint8 -> (H, W) uint8: min over the (2r + 1)^2 window clipped to the image of min(R, G, B); separable, by shifted slices"""
    m = np.asarray(img).min(axis=-1)
    H, W = m.shape
    rows = m.copy()
    for d in range(1, min(r, W - 1) + 1):
        rows[:, d:] = np.minimum(rows[:, d:], m[:, :W - d])
        rows[:, :W - d] = np.minimum(rows[:, :W - d], m[:, d:])
    out = rows.copy()
    for d in range(1, min(r, H - 1) + 1):
        out[d:, :] = np.minimum(out[d:, :], rows[:H - d, :])
        out[:H - d, :] = np.minimum(out[:H - d, :], rows[d:, :])
    return out


def gradient_sum(Y):
    """(H, W) int64 -> float64: sum over the (H-1)(W-1) positions of sqrt(0.5 (dx^2 + dy^2)), forward differences"""
    if Y.shape[0] < 2 or Y.shape[1] < 2:
        return 0.0
    dx = Y[:-1, 1:] - Y[:-1, :-1]
    dy = Y[1:, :-1] - Y[:-1, :-1]
    return float(np.sqrt(0.5 * (dx * dx + dy * dy).astype(np.float64)).sum())


def stats(hazy, out, r):
    """(B, H, W, 3) uint8 pair -> counts (B, 2, 259) int64, grad (B, 2) float64, dark maps (2, B, H, W) uint8: the outputs of cfen_noref_u8"""
    hazy, out = np.asarray(hazy), np.asarray(out)
    assert hazy.shape == out.shape and hazy.dtype == np.uint8 == out.dtype and hazy.ndim == 4 and hazy.shape[3] == 3 and 0 <= r <= 16
    B, H, W, _ = hazy.shape
    counts = np.zeros((B, 2, 259), np.int64)
    grad = np.zeros((B, 2), np.float64)
    maps = np.zeros((2, B, H, W), np.uint8)
    for b in range(B):
        Ys = []
        for s, img in enumerate((hazy[b], out[b])):
            Y = luma(img)
            Ys.append(Y)
            maps[s, b] = dark_channel(img, r)
            counts[b, s, :256] = np.bincount(Y.ravel(), minlength=256)
            counts[b, s, 256] = int(maps[s, b].astype(np.int64).sum())
            grad[b, s] = gradient_sum(Y)
        sat_h = (Ys[0] == 0) | (Ys[0] == 255)
        sat_o = (Ys[1] == 0) | (Ys[1] == 255)
        counts[b, 0, 257] = int(sat_h.sum())
        counts[b, 1, 257] = int((sat_o & ~sat_h).sum())
    return counts, grad, maps


def scores_from_stats(counts, grad, H, W):
    """(B, 9) float64 in the order of COLUMNS"""
    counts, grad = np.asarray(counts), np.asarray(grad)
    n = float(H * W)
    rows = []
    for c, g in zip(counts, grad):
        side = []
        for s in range(2):
            p = c[s, :256].astype(np.float64) / n
            nz = p[p > 0]
            v = np.arange(256, dtype=np.float64) / 255.0
            mean = (p * v).sum()
            side.append((c[s, 256] / (255.0 * n), float(-(nz * np.log2(nz)).sum()) + 0.0,
                         g[s] / ((H - 1) * (W - 1)) if (H - 1) * (W - 1) > 0 else float("nan"), float(np.sqrt((p * (v - mean) ** 2).sum()))))
        a, b = side
        rows.append((a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], c[1, 257] / n))
    return np.array(rows, np.float64)


def scores(hazy, out, r):
    counts, grad, _ = stats(hazy, out, r)
    return scores_from_stats(counts, grad, hazy.shape[1], hazy.shape[2])


# ---- brute force, for small images ------------------------------------------------------------------------------------------------------------------
def brute_force(hazy, out, r):
    """the definition as a double loop over pixels and windows, Python integers; (counts, grad, maps) as stats()"""
    import math
    hazy, out = np.asarray(hazy), np.asarray(out)
    B, H, W, _ = hazy.shape
    counts = np.zeros((B, 2, 259), np.int64)
    grad = np.zeros((B, 2), np.float64)
    maps = np.zeros((2, B, H, W), np.uint8)
    for b in range(B):
        Y = [[[(77 * int(img[y, x, 0]) + 150 * int(img[y, x, 1]) + 29 * int(img[y, x, 2]) + 128) >> 8 for x in range(W)] for y in range(H)]
             for img in (hazy[b], out[b])]
        for s, img in enumerate((hazy[b], out[b])):
            for y in range(H):
                for x in range(W):
                    d = 255
                    for yy in range(max(0, y - r), min(H, y + r + 1)):
                        for xx in range(max(0, x - r), min(W, x + r + 1)):
                            d = min(d, int(img[yy, xx, 0]), int(img[yy, xx, 1]), int(img[yy, xx, 2]))
                    maps[s, b, y, x] = d
                    counts[b, s, 256] += d
                    counts[b, s, Y[s][y][x]] += 1
                    if y + 1 < H and x + 1 < W:
                        dx, dy = Y[s][y][x + 1] - Y[s][y][x], Y[s][y + 1][x] - Y[s][y][x]
                        grad[b, s] += math.sqrt(0.5 * (dx * dx + dy * dy))
        for y in range(H):
            for x in range(W):
                sh, so = Y[0][y][x] in (0, 255), Y[1][y][x] in (0, 255)
                counts[b, 0, 257] += sh
                counts[b, 1, 257] += so and not sh
    return counts, grad, maps


# ---- the cases of the device tests ------------------------------------------------------------------------------------------------------------------
def _random(shape, rs):
    return rs.randint(0, 256, shape + (3,), dtype=np.uint8), rs.randint(0, 256, shape + (3,), dtype=np.uint8)


def _constant(shape, rs):
    return np.full(shape + (3,), 93, np.uint8), np.full(shape + (3,), 200, np.uint8)


def _black_white(shape, rs):
    """image 0: all 0 -> all 255 (already saturated: sat_in = H W, sat_new = 0); image 1: grey 128 -> all 255 (sat_new = H W); last: 255 -> 0"""
    hazy, out = np.zeros(shape + (3,), np.uint8), np.full(shape + (3,), 255, np.uint8)
    if shape[0] > 1:
        hazy[1] = 128
    if shape[0] > 2:
        hazy[2], out[2] = 255, 0
    return hazy, out


def _ramp(shape, rs):
    B, H, W = shape
    x = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)
    hazy = np.broadcast_to(x[None, None, :, None], shape + (3,)).copy()
    out = hazy[:, :, ::-1].copy()
    out[..., 1] //= 2
    return hazy, out


DOT_AT = ((60, 66), (0, 0))          # the dark pixels of the dot case: one across a tile corner, one in the image's corner


def _dot(shape, rs):
    hazy = np.full(shape + (3,), 255, np.uint8)
    out = np.full(shape + (3,), 255, np.uint8)
    for b in range(shape[0]):
        y, x = DOT_AT[b % len(DOT_AT)]
        hazy[b, y, x] = (255, 0, 255)           # one channel is enough to be dark
        out[b, shape[1] - 1 - y, shape[2] - 1 - x] = (7, 9, 8)
    return hazy, out


# name -> (generator, (B, H, W), r)
CASES = {
    "1x1x1_r7": (_random, (1, 1, 1), 7),                                     # the smallest input: no gradient position
    "2x3x5_r7": (_random, (2, 3, 5), 7),                                     # smaller than the window
    "3x17x67_r7": (_random, (3, 17, 67), 7),                                 # image stride 3417 bytes: images 1 and 2 start misaligned; two tiles across
    "1x64x64_r0": (_random, (1, 64, 64), 0),
    "1x64x64_r1": (_random, (1, 64, 64), 1),
    "1x64x64_r7": (_random, (1, 64, 64), 7),
    "1x64x64_r16": (_random, (1, 64, 64), 16),
    "2x97x131_r7": (_random, (2, 97, 131), 7),                               # 2 x 3 tiles, odd sizes, image 1 misaligned
    "w_tile-1_r16": (_random, (1, 70, TILE_W - 1), 16),                      # a halo of 16 across every tile edge
    "w_tile_r16": (_random, (1, 70, TILE_W), 16),
    "w_tile+1_r16": (_random, (1, 70, TILE_W + 1), 16),
    "h_tile-1_r16": (_random, (1, TILE_H - 1, 70), 16),
    "h_tile_r16": (_random, (1, TILE_H, 70), 16),
    "h_tile+1_r16": (_random, (1, TILE_H + 1, 70), 16),
    "1x1025x1023_r7": (_random, (1, 16 * TILE_H + 1, 16 * TILE_W - 1), 7),   # 17 x 16 = 272 records: more than the finish workgroup has threads
    "1x1x70_r7": (_random, (1, 1, 70), 7),                                   # H == 1: gradient sum 0
    "constant_r7": (_constant, (1, 70, 75), 7),                              # every lane on one histogram bin
    "black_white_r7": (_black_white, (3, 70, 75), 7),
    "ramp_r7": (_ramp, (1, 70, 131), 7),
    "dot_r16": (_dot, (2, 100, 100), 16),
    "dot_r7": (_dot, (2, 100, 100), 7),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(hazy, out, r, counts, grad, maps): computed once, shared, read-only"""
    gen, shape, r = CASES[name]
    hazy, out = gen(shape, np.random.RandomState(sum(shape) + 31 * r + len(name)))
    assert hazy.shape == shape + (3,) == out.shape
    counts, grad, maps = stats(hazy, out, r)
    for x in (hazy, out, counts, grad, maps):
        x.setflags(write=False)
    return hazy, out, r, counts, grad, maps
