"""numpy application of the product's resampling tables (cfen_vit_dehazing_amd/resample.py) to uint8 arrays: what csrc/k_resample.hip computes,
restated for the host tests.  The product itself has no CPU path."""
import numpy as np

from cfen_vit_dehazing_amd import resample


def apply_pass(src, bounds, coef, axis):
    """one pass along `axis` of a (..., H, W, C) uint8 array (axis = -2: horizontal, -3: vertical): int32 sums, arithmetic shift, clip"""
    src = np.moveaxis(src, axis, 0)
    out = np.empty((bounds.shape[0],) + src.shape[1:], dtype=np.uint8)
    for xx in range(bounds.shape[0]):
        xmin, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        k = coef[xx, :n].astype(np.int32).reshape((n,) + (1,) * (src.ndim - 1))
        acc = (src[xmin:xmin + n].astype(np.int32) * k).sum(axis=0, dtype=np.int32) + np.int32(1 << 21)
        out[xx] = np.clip(acc >> 22, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(src, size, filter="bicubic"):
    """Image.resize((W2, H2)) of a (..., H, W, 3) uint8 array; size = (H2, W2)"""
    H, W = src.shape[-3], src.shape[-2]
    H2, W2 = size
    out = src
    if W2 != W:
        out = apply_pass(out, *resample.coefficients(W, W2, filter), axis=-2)
    if H2 != H:
        out = apply_pass(out, *resample.coefficients(H, H2, filter), axis=-3)
    return out.copy() if out is src else out


PIL_FILTER = {"bicubic": "BICUBIC", "bilinear": "BILINEAR", "box": "BOX", "hamming": "HAMMING", "lanczos": "LANCZOS"}


def pil_resize(a, size, filter="bicubic"):
    """the reference of every comparison: PIL as installed; a: (H,W,3) uint8, size = (H2, W2)"""
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((size[1], size[0]), getattr(Image, PIL_FILTER[filter])))
