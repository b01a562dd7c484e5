"""CIEDE2000 of 8-bit sRGB images in float64 numpy: the restatement of include/cfen_colordiff.h that tests/test_ciede_host.py checks against
published values and tests/test_hip_ciede.py holds the device kernel to.  Nothing here is rounded to fp32: the table and the matrix are the
fp64 values whose fp32 roundings the kernel uses."""
import itertools

import numpy as np

M = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]], np.float64)
MN = M / ((M[:, 0] + M[:, 1]) + M[:, 2])[:, None]          # each row divided by its own sum: the matrix's own white is (1, 1, 1)
POW25_7 = 25.0 ** 7


def srgb_linear_table():
    """lin[v], v = 0 .. 255, float64"""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


def lab_from_bytes(u8):
    """(..., 3) uint8 -> (L, a, b), float64; a pixel with R = G = B has a = b = 0 exactly"""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.shape[-1] == 3
    lin = srgb_linear_table()[u8]
    t = [(MN[i, 0] * lin[..., 0] + MN[i, 1] * lin[..., 1]) + MN[i, 2] * lin[..., 2] for i in range(3)]
    d = 6.0 / 29.0
    fx, fy, fz = (np.where(v > d ** 3, np.cbrt(v), v * (841.0 / 108.0) + 4.0 / 29.0) for v in t)
    grey = (u8[..., 0] == u8[..., 1]) & (u8[..., 1] == u8[..., 2])
    return 116.0 * fy - 16.0, np.where(grey, 0.0, 500.0 * (fx - fy)), np.where(grey, 0.0, 200.0 * (fy - fz))


def _hue(b, ap):
    h = np.degrees(np.arctan2(b, ap))
    h = np.where(h < 0, h + 360.0, h)
    return np.where((ap == 0) & (b == 0), 0.0, h)


def delta_e_terms(L1, a1, b1, L2, a2, b2, hbar_other=False, dh_other=False):
    """Sharma, Wu and Dalal (2005), kL = kC = kH = 1 -> (dE00, h1', h2', C1' C2').  hbar_other: the mean hue on the other side of the circle
    (hbar' + 180 below 180, hbar' - 180 from there on); dh_other: the hue difference the other way round (dh' - 360 if positive, else + 360).
    With both False it is the formula."""
    L1, a1, b1, L2, a2, b2 = (np.asarray(v, np.float64) for v in (L1, a1, b1, L2, a2, b2))
    C1, C2 = np.sqrt(a1 * a1 + b1 * b1), np.sqrt(a2 * a2 + b2 * b2)
    c7 = (0.5 * (C1 + C2)) ** 7
    G = 0.5 * (1.0 - np.sqrt(c7 / (c7 + POW25_7)))
    a1p, a2p = (1.0 + G) * a1, (1.0 + G) * a2
    C1p, C2p = np.sqrt(a1p * a1p + b1 * b1), np.sqrt(a2p * a2p + b2 * b2)
    h1, h2 = _hue(b1, a1p), _hue(b2, a2p)
    dL, dC = L2 - L1, C2p - C1p
    CC = C1p * C2p
    z = CC == 0
    dh = h2 - h1
    dh = np.where(dh > 180.0, dh - 360.0, np.where(dh < -180.0, dh + 360.0, dh))
    if dh_other:
        dh = np.where(dh > 0, dh - 360.0, dh + 360.0)
    dh = np.where(z, 0.0, dh)
    dH = 2.0 * np.sqrt(CC) * np.sin(np.radians(0.5 * dh))
    Lb, Cb = 0.5 * (L1 + L2), 0.5 * (C1p + C2p)
    hs = h1 + h2
    hb = np.where(np.abs(h1 - h2) <= 180.0, 0.5 * hs, np.where(hs < 360.0, 0.5 * (hs + 360.0), 0.5 * (hs - 360.0)))
    if hbar_other:
        hb = np.where(hb < 180.0, hb + 180.0, hb - 180.0)
    hb = np.where(z, hs, hb)
    T = (1.0 - 0.17 * np.cos(np.radians(hb - 30.0)) + 0.24 * np.cos(np.radians(2.0 * hb)) + 0.32 * np.cos(np.radians(3.0 * hb + 6.0))
         - 0.20 * np.cos(np.radians(4.0 * hb - 63.0)))
    dth = 30.0 * np.exp(-(((hb - 275.0) / 25.0) ** 2))
    cb7 = Cb ** 7
    Rc = 2.0 * np.sqrt(cb7 / (cb7 + POW25_7))
    l50 = (Lb - 50.0) ** 2
    Sl, Sc, Sh = 1.0 + 0.015 * l50 / np.sqrt(20.0 + l50), 1.0 + 0.045 * Cb, 1.0 + 0.015 * Cb * T
    Rt = -np.sin(np.radians(2.0 * dth)) * Rc
    tl, tc, th = dL / Sl, dC / Sc, dH / Sh
    return np.sqrt(np.maximum(tl * tl + tc * tc + th * th + Rt * tc * th, 0.0)), h1, h2, CC


def delta_e_lab(L1, a1, b1, L2, a2, b2):
    return delta_e_terms(L1, a1, b1, L2, a2, b2)[0]


def ciede2000_u8(a, b):
    """per-pixel dE00 of two (..., 3) uint8 sRGB images, float64, a as colour 1 and b as colour 2"""
    return delta_e_lab(*(lab_from_bytes(a) + lab_from_bytes(b)))


def branch_values(a, b):
    """(4, ...) float64: what the formula gives for the pixel pairs with hbar' or the opposite mean hue, and with dh' or the other way round --
    the values a pixel at the discontinuity (hues exactly opposite) may legitimately take.  Row 0 is the formula itself."""
    lab = lab_from_bytes(a) + lab_from_bytes(b)
    return np.stack([delta_e_terms(*lab, hbar_other=hb, dh_other=dh)[0] for hb in (False, True) for dh in (False, True)])


def opposite_hues(a, b, tol_deg=0.01):
    """mask of the pixel pairs the discontinuity can reach: both colours chromatic and ||h1' - h2'| - 180| < tol_deg, in float64"""
    _, h1, h2, CC = delta_e_terms(*(lab_from_bytes(a) + lab_from_bytes(b)))
    return (CC != 0) & (np.abs(np.abs(h1 - h2) - 180.0) < tol_deg)


CORNER_LEVELS = (0, 1, 2, 127, 128, 129, 254, 255)


def corner_grid():
    """the 512 colours with every channel in CORNER_LEVELS, in itertools.product order, as a 512 x 512 image pair: pixel (i, j) is
    (colour i, colour j)"""
    c = np.array(list(itertools.product(CORNER_LEVELS, repeat=3)), np.uint8)
    n = len(c)
    return np.ascontiguousarray(np.broadcast_to(c[:, None, :], (n, n, 3))), np.ascontiguousarray(np.broadcast_to(c[None, :, :], (n, n, 3)))


# Sharma, Wu and Dalal (2005), table 1: L1 a1 b1  L2 a2 b2  dE00 -- public test data of the paper
SHARMA = np.array([[float(x) for x in line.split()] for line in """\
50.0000 2.6772 -79.7751 50.0000 0.0000 -82.7485 2.0425
50.0000 3.1571 -77.2803 50.0000 0.0000 -82.7485 2.8615
50.0000 2.8361 -74.0200 50.0000 0.0000 -82.7485 3.4412
50.0000 -1.3802 -84.2814 50.0000 0.0000 -82.7485 1.0000
50.0000 -1.1848 -84.8006 50.0000 0.0000 -82.7485 1.0000
50.0000 -0.9009 -85.5211 50.0000 0.0000 -82.7485 1.0000
50.0000 0.0000 0.0000 50.0000 -1.0000 2.0000 2.3669
50.0000 -1.0000 2.0000 50.0000 0.0000 0.0000 2.3669
50.0000 2.4900 -0.0010 50.0000 -2.4900 0.0009 7.1792
50.0000 2.4900 -0.0010 50.0000 -2.4900 0.0010 7.1792
50.0000 2.4900 -0.0010 50.0000 -2.4900 0.0011 7.2195
50.0000 2.4900 -0.0010 50.0000 -2.4900 0.0012 7.2195
50.0000 -0.0010 2.4900 50.0000 0.0009 -2.4900 4.8045
50.0000 -0.0010 2.4900 50.0000 0.0010 -2.4900 4.8045
50.0000 -0.0010 2.4900 50.0000 0.0011 -2.4900 4.7461
50.0000 2.5000 0.0000 50.0000 0.0000 -2.5000 4.3065
50.0000 2.5000 0.0000 73.0000 25.0000 -18.0000 27.1492
50.0000 2.5000 0.0000 61.0000 -5.0000 29.0000 22.8977
50.0000 2.5000 0.0000 56.0000 -27.0000 -3.0000 31.9030
50.0000 2.5000 0.0000 58.0000 24.0000 15.0000 19.4535
50.0000 2.5000 0.0000 50.0000 3.1736 0.5854 1.0000
50.0000 2.5000 0.0000 50.0000 3.2972 0.0000 1.0000
50.0000 2.5000 0.0000 50.0000 1.8634 0.5757 1.0000
50.0000 2.5000 0.0000 50.0000 3.2592 0.3350 1.0000
60.2574 -34.0099 36.2677 60.4626 -34.1751 39.4387 1.2644
63.0109 -31.0961 -5.8663 62.8187 -29.7946 -4.0864 1.2630
61.2901 3.7196 -5.3901 61.4292 2.2480 -4.9620 1.8731
35.0831 -44.1164 3.7933 35.0232 -40.0716 1.5901 1.8645
22.7233 20.0904 -46.6940 23.0331 14.9730 -42.5619 2.0373
36.4612 47.8580 18.3852 36.2715 50.5065 21.2231 1.4146
90.8027 -2.0831 1.4410 91.1528 -1.6435 0.0447 1.4441
90.9257 -0.5406 -0.9208 88.6381 -0.8985 -0.7239 1.5381
6.7747 -0.2908 -2.4247 5.8714 -0.0985 -2.2286 0.6377
2.0776 0.0795 -1.1350 0.9033 -0.0636 -0.5514 0.9082""".splitlines()])
