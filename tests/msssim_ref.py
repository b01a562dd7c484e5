"""Image pairs and the float64 restatement behind tests/golden/msssim_pairs.npz (tools/gen_golden_msssim.py, test_msssim_host.py,
test_hip_msssim.py).

Definition (include/cfen_hip.h, cfen_image_msssim): the reference's pytorch_msssim.msssim(window_size=11, size_average=True, val_range=1,
normalize=None).  Level 0 is the image on the [0,1] scale, level l + 1 the mean of each 2 x 2 block of level l (odd sizes floor: the last row /
column is dropped); at every level the 11 x 11 Gaussian window as a valid convolution gives the mean SSIM and the mean of
cs = (2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2); MS-SSIM = prod_{l<4} cs_l^w_l * ssim_4^w_4, NaN when a used term is negative.

The images are not stored: `pair(name)` regenerates them with the integer generator of metrics_images.pair (same recipe, other seeds and
sizes), so they are bit-identical on every machine; the fixture's CRC32s prove it."""
import numpy as np

import metrics_images as mi

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
LEVELS = 5
MIN_EDGE = 176                       # level 4 must still hold one 11 x 11 window: 11 * 2^4

# name -> (batch, H, W, seed, kind)
CASES = {
    "176x176": (1, 176, 176, 201, "noisy"),
    "177x203_batch2": (2, 177, 203, 202, "noisy"),
    "200x330": (1, 200, 330, 203, "noisy"),
    "512x512_batch8": (8, 512, 512, 204, "noisy"),
    "identical_176": (1, 176, 176, 205, "identical"),
    "black_white_176": (1, 176, 176, 206, "black_white"),
    "anticorrelated_176": (1, 176, 176, 207, "anticorrelated"),
}


def pair(name):
    """(a, b): two (B,H,W,3) uint8 arrays.  noisy / identical / black_white: the recipe of metrics_images.pair (b a 'clear' image of 8 x 8 blocks
    plus fine noise, a = b with a veil, less contrast and more noise).  anticorrelated: a is fine noise over the whole byte range, b = 255 - a"""
    B, H, W, seed, kind = CASES[name]
    rs = np.random.RandomState(seed)
    a = np.empty((B, H, W, 3), dtype=np.uint8)
    b = np.empty((B, H, W, 3), dtype=np.uint8)
    for i in range(B):
        if kind == "black_white":
            a[i], b[i] = 0, 255
            continue
        if kind == "anticorrelated":
            a[i] = rs.randint(0, 256, (H, W, 3))
            b[i] = 255 - a[i].astype(np.int64)
            continue
        clear = np.clip(mi._image(rs, H, W, 8) + rs.randint(-12, 13, (H, W, 3)), 0, 255)
        b[i] = clear
        if kind == "identical":
            a[i] = clear
            continue
        veil = 40 + 10 * i
        a[i] = np.clip(clear * 3 // 4 + veil + rs.randint(-6, 7, (H, W, 3)), 0, 255)
    return a, b


def pool2(x):
    """mean of each 2 x 2 block of (..., H, W); an odd last row / column is dropped (F.avg_pool2d(x, (2, 2)))"""
    H, W = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    x = x[..., :H, :W]
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) * 0.25


def ssim_cs_f64(a01, b01):
    """(mean SSIM, mean cs) of two (C,H,W) float64 images on the [0,1] scale, over every channel and window position"""
    w = mi.gaussian_window()
    mu1, mu2 = mi._filter_valid(a01, w), mi._filter_valid(b01, w)
    s11 = mi._filter_valid(a01 * a01, w) - mu1 * mu1
    s22 = mi._filter_valid(b01 * b01, w) - mu2 * mu2
    s12 = mi._filter_valid(a01 * b01, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    v1, v2 = 2 * s12 + C2, s11 + s22 + C2
    m = ((2 * mu1 * mu2 + C1) * v1) / ((mu1 * mu1 + mu2 * mu2 + C1) * v2)
    return float(m.mean()), float((v1 / v2).mean())


def levels_f64(a01, b01):
    """(5, 2) float64: (ssim_l, cs_l) of two (C,H,W) images on the [0,1] scale, min(H, W) >= 176"""
    a01, b01 = np.asarray(a01, dtype=np.float64), np.asarray(b01, dtype=np.float64)
    if min(a01.shape[-2:]) < MIN_EDGE:
        raise ValueError("MS-SSIM over five levels needs min(H, W) >= %d, got %d x %d" % ((MIN_EDGE,) + tuple(a01.shape[-2:])))
    out = np.empty((LEVELS, 2), dtype=np.float64)
    for l in range(LEVELS):
        out[l] = ssim_cs_f64(a01, b01)
        a01, b01 = pool2(a01), pool2(b01)
    return out


def levels_f64_u8(a, b):
    """two (H,W,3) uint8 images"""
    return levels_f64(a.transpose(2, 0, 1).astype(np.float64) / 255.0, b.transpose(2, 0, 1).astype(np.float64) / 255.0)


def combine(levels):
    """MS-SSIM of one (5, 2) array of level values in float64; NaN when cs_0 .. cs_3 or ssim_4 is negative"""
    levels = np.asarray(levels, dtype=np.float64)
    terms = list(levels[:LEVELS - 1, 1]) + [levels[LEVELS - 1, 0]]
    if min(terms) < 0:
        return float("nan")
    return float(np.prod([t ** w for t, w in zip(terms, WEIGHTS)]))
