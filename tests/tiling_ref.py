"""float64 numpy restatement of the tile plan, gather and blend of overlapping-tile inference (cfen_vit_dehazing_amd/tiled.py), written from
the definitions in its docstring; used by test_tiling_plan.py (CPU) and test_hip_tiled.py (GPU)."""
import math

import numpy as np


def n_tiles(L, T, o):
    return 1 if L <= T else 1 + math.ceil((L - T) / (T - o))


def origins(L, T, o):
    n = n_tiles(L, T, o)
    return [0] if n == 1 else [(j * (L - T)) // (n - 1) for j in range(n)]


def mirror(k, L):
    """numpy 'reflect' of index array k into [0, L)"""
    k = np.asarray(k)
    if L == 1:
        return np.zeros_like(k)
    period = 2 * (L - 1)
    k = np.mod(k, period)
    return np.where(k < L, k, period - k)


def gather(img, T, o, hwc):
    """all tiles of img ((H,W,C) if hwc else (C,H,W)) in row-major order: (n, T, T, C) or (n, C, T, T)"""
    H, W = (img.shape[0], img.shape[1]) if hwc else (img.shape[1], img.shape[2])
    out = []
    for p in origins(H, T, o):
        rows = mirror(p + np.arange(T), H)
        for q in origins(W, T, o):
            cols = mirror(q + np.arange(T), W)
            out.append(img[rows][:, cols] if hwc else img[:, rows][:, :, cols])
    return np.stack(out)


def axis_weight(T, L, o):
    e = min(T, L)
    u = np.arange(e)
    d = np.minimum(u, e - 1 - u)
    return np.minimum(1.0, (d + 1) / (o + 1))


def blend(tiles, H, W, T, o):
    """tiles (n, C, T, T) in row-major tile order -> ((C,H,W) float64 blended image, (H,W) count of covering tiles)"""
    tiles = np.asarray(tiles, dtype=np.float64)
    C = tiles.shape[1]
    num = np.zeros((C, H, W))
    den = np.zeros((H, W))
    cnt = np.zeros((H, W), dtype=np.int64)
    first = np.zeros((C, H, W))
    wy_all, wx_all = axis_weight(T, H, o), axis_weight(T, W, o)
    t = 0
    for p in origins(H, T, o):
        hy = min(T, H - p)
        for q in origins(W, T, o):
            hx = min(T, W - q)
            v = tiles[t, :, :hy, :hx]
            w = wy_all[:hy, None] * wx_all[None, :hx]
            sl = (slice(p, p + hy), slice(q, q + hx))
            num[(slice(None),) + sl] += w * v
            den[sl] += w
            fresh = cnt[sl] == 0
            first[(slice(None),) + sl] = np.where(fresh, v, first[(slice(None),) + sl])
            cnt[sl] += 1
            t += 1
    out = np.where(cnt == 1, first, num / np.maximum(den, 1e-300))
    return out, cnt
