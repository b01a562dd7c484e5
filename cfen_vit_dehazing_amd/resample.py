"""Integer tables of PIL's 8-bit resampling (`Image.resize` on uint8 images; libImaging/Resample.c), built on the host in numpy.

PIL resamples 8-bit images in fixed point: per axis the double-precision filter weights are normalised, rounded ONCE to 22-bit integers, and every
output byte is clip((2^21 + sum_x src[xmin + x] * k_x) >> 22, 0, 255) in int32; the horizontal pass is stored as uint8 before the vertical pass reads
it.  `coefficients` builds (bounds, coef) in PIL's order of operations; the device pass (csrc/k_resample.hip, ops.resample_u8) is integers only, so
bitwise equality with PIL does not depend on any floating-point behaviour of the device.  tests/test_resample_host.py sweeps these tables, applied
by tests/resample_ref.py, against the installed PIL byte for byte.
"""
import math

import numpy as np

PRECISION_BITS = 22          # 32 - 8 - 2 (Resample.c)

FILTER_SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "box": 0.5, "hamming": 1.0, "lanczos": 3.0}
FILTERS = tuple(FILTER_SUPPORT)          # every one passes the bitwise sweep


def _sin(a):
    """math.sin per element: the C library's sin, what PIL calls (np.sin may be a vectorised implementation with other last bits)"""
    return np.array([math.sin(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def _cos(a):
    return np.array([math.cos(v) for v in a.ravel()], dtype=np.float64).reshape(a.shape)


def _sinc(x):
    px = x * math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x == 0.0, 1.0, _sin(px) / px)


def _filter(name, x):
    """the filter on a float64 array, operation for operation as Resample.c evaluates it on one double"""
    if name == "box":
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    if name == "lanczos":
        return np.where((x >= -3.0) & (x < 3.0), _sinc(x) * _sinc(x / 3), 0.0)
    x = np.abs(x)
    if name == "bilinear":
        return np.where(x < 1.0, 1.0 - x, 0.0)
    if name == "hamming":
        px = x * math.pi
        with np.errstate(divide="ignore", invalid="ignore"):
            w = _sin(px) / px * (float(np.float32(0.54)) + float(np.float32(0.46)) * _cos(px))          # (0.54f, 0.46f in Resample.c)
        return np.where(x == 0.0, 1.0, np.where(x >= 1.0, 0.0, w))
    if name == "bicubic":
        a = -0.5
        return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    raise ValueError("unknown resampling filter %r (one of %s)" % (name, ", ".join(FILTERS)))


_TABLES = {}


def coefficients(in_size, out_size, filter="bicubic"):
    """(bounds int32 (out, 2), coef int32 (out, ksize)) of one axis: output index xx reads source indices bounds[xx, 0] + (0 .. bounds[xx, 1] - 1) with
    the weights coef[xx, :bounds[xx, 1]] (scaled by 2^22); coef[xx, bounds[xx, 1]:] = 0.  ValueError for a table whose int32 sum could overflow."""
    in_size, out_size = int(in_size), int(out_size)
    key = (in_size, out_size, filter)
    if key in _TABLES:
        return _TABLES[key]
    if filter not in FILTER_SUPPORT:
        raise ValueError("unknown resampling filter %r (one of %s)" % (filter, ", ".join(FILTERS)))
    if in_size < 1 or out_size < 1:
        raise ValueError("resample: sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(0, np.trunc(center - support + 0.5).astype(np.int64))
    xmax = np.minimum(in_size, np.trunc(center + support + 0.5).astype(np.int64))
    n = xmax - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    live = x < n[:, None]
    # (x + xmin) is an int sum in C, converted to double, then - center, + 0.5, * ss: the same order here
    w = np.where(live, _filter(filter, ((x + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for t in range(ksize):          # the sum runs left to right (the zeros past n leave it unchanged)
        ww = ww + w[:, t]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where((ww != 0.0)[:, None], w / ww[:, None], w)
    w = np.where(live, w, 0.0)
    coef = np.trunc(np.where(w < 0, w * (1 << PRECISION_BITS) - 0.5, w * (1 << PRECISION_BITS) + 0.5)).astype(np.int64)
    worst = int(np.abs(coef).sum(axis=1).max())
    if 255 * worst + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise ValueError("resample %d -> %d (%s): a row of the table sums to %d / 2^22 in magnitude; 255 times that does not fit the int32 "
                         "accumulator" % (in_size, out_size, filter, worst))
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    coef = np.ascontiguousarray(coef.astype(np.int32))
    bounds.setflags(write=False)
    coef.setflags(write=False)
    if len(_TABLES) >= 64:
        _TABLES.clear()
    _TABLES[key] = (bounds, coef)
    return bounds, coef


_DEVICE_TABLES = {}


def device_tables(in_size, out_size, filter, device):
    """(bounds, coef) of `coefficients` as int32 tensors on `device`, uploaded once per (in, out, filter, device)"""
    import torch
    device = torch.device(device)
    key = (int(in_size), int(out_size), filter, device.type, device.index)
    if key not in _DEVICE_TABLES:
        bounds, coef = coefficients(in_size, out_size, filter)
        if len(_DEVICE_TABLES) >= 64:
            _DEVICE_TABLES.clear()
        _DEVICE_TABLES[key] = (torch.from_numpy(bounds.copy()).to(device), torch.from_numpy(coef.copy()).to(device))
    return _DEVICE_TABLES[key]
