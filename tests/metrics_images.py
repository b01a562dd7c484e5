"""Image pairs and the float64 restatement behind tests/golden/metrics_pairs.npz (tools/gen_golden_metrics.py, test_metrics_host.py,
test_hip_metrics.py).

The images are not stored: `pair(name)` regenerates them from np.random.RandomState(seed) with integer arithmetic only (randint blocks enlarged
with np.kron, randint noise, clip), so they are bit-identical on every machine; the fixture's CRC32s prove it.

`ssim_f64` / `sse_int` / `psnr_from_sse` restate the definition of include/cfen_hip.h (cfen_image_metrics) in float64 numpy."""
import math
import zlib

import numpy as np

# name -> (batch, H, W, seed, kind)
CASES = {
    "11x11": (1, 11, 11, 101, "noisy"),
    "37x53": (1, 37, 53, 102, "noisy"),
    "64x64": (1, 64, 64, 103, "noisy"),
    "512x512_batch8": (8, 512, 512, 104, "noisy"),
    "480x640": (1, 480, 640, 105, "noisy"),
    "1080x1920": (1, 1080, 1920, 106, "noisy"),
    "identical_64x64": (1, 64, 64, 107, "identical"),
    "black_white_64x64": (1, 64, 64, 108, "black_white"),
}


def _image(rs, H, W, block):
    coarse = rs.randint(0, 256, (-(-H // block), -(-W // block), 3)).astype(np.int64)
    return np.kron(coarse, np.ones((block, block, 1), dtype=np.int64))[:H, :W]


def pair(name):
    """(a, b): two (B,H,W,3) uint8 arrays -- b a 'clear' image (blocks of 8 plus fine noise), a = b with a veil, less contrast and more noise"""
    B, H, W, seed, kind = CASES[name]
    rs = np.random.RandomState(seed)
    a = np.empty((B, H, W, 3), dtype=np.uint8)
    b = np.empty((B, H, W, 3), dtype=np.uint8)
    for i in range(B):
        if kind == "black_white":
            a[i], b[i] = 0, 255
            continue
        clear = np.clip(_image(rs, H, W, 8) + rs.randint(-12, 13, (H, W, 3)), 0, 255)
        b[i] = clear
        if kind == "identical":
            a[i] = clear
            continue
        veil = 40 + 10 * i                                     # integer haze: clear * 3 // 4 + veil, then noise
        a[i] = np.clip(clear * 3 // 4 + veil + rs.randint(-6, 7, (H, W, 3)), 0, 255)
    return a, b


def crc(x):
    return zlib.crc32(np.ascontiguousarray(x).tobytes()) & 0xFFFFFFFF


def gaussian_window(dtype=np.float64):
    g = np.array([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=np.float64)
    return (g / g.sum()).astype(dtype)


def _filter_valid(x, w):
    """separable 11-tap valid filter of (..., H, W) along the last two axes"""
    H, W = x.shape[-2:]
    rows = sum(w[j] * x[..., :, j:j + W - 10] for j in range(11))
    return sum(w[j] * rows[..., j:j + H - 10, :] for j in range(11))


def ssim_f64(a01, b01):
    """mean SSIM of two (C,H,W) float64 images on the [0,1] scale: 11 x 11 Gaussian window (sigma 1.5), valid convolution, C1 = 0.01^2,
    C2 = 0.03^2, the mean over every channel and window position"""
    a01, b01 = np.asarray(a01, dtype=np.float64), np.asarray(b01, dtype=np.float64)
    w = gaussian_window()
    mu1, mu2 = _filter_valid(a01, w), _filter_valid(b01, w)
    s11 = _filter_valid(a01 * a01, w) - mu1 * mu1
    s22 = _filter_valid(b01 * b01, w) - mu2 * mu2
    s12 = _filter_valid(a01 * b01, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    return float(m.mean())


def ssim_f64_u8(a, b):
    """two (H,W,3) uint8 images"""
    return ssim_f64(a.transpose(2, 0, 1).astype(np.float64) / 255.0, b.transpose(2, 0, 1).astype(np.float64) / 255.0)


def sse_int(a, b):
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def psnr_from_sse(sse, n):
    """10 log10(255^2 n / sse) over n values, inf for equal images"""
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n / sse)
