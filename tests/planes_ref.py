"""The definition of include/cfen_planes.h (cfen_plane_metrics; ops.plane_metrics, gtscore.Scorer, dehaze_video.py --eval_gt) restated in numpy,
and the seeded frame pairs its tests share (tests/test_planes_host.py, tests/test_hip_plane_metrics.py, tests/test_hip_video_gt.py).

A frame is a y4m payload: uint8 bytes, one per sample at depth 8, two little-endian bytes at depths 9 .. 16.  `words` returns what the device
writes per frame and plane: SSE and DT as exact Python / int64 integers, the mean SSIM in float64 (metrics_images.ssim_f64 on the plane divided
by top: the float64 restatement the device's fp32 map arithmetic is held against), the sample count."""
import functools
import math

import numpy as np

import metrics_images as mi
import yuv_ref

CHROMAS = yuv_ref.CHROMAS


def top(depth):
    return (1 << depth) - 1


def plane_shapes(H, W, chroma):
    """[(h, w)] of the planes the format has: Y alone for mono, else Y, Cb, Cr"""
    hc, wc = yuv_ref.chroma_shape(H, W, chroma)
    return [(H, W)] if chroma == "mono" else [(H, W), (hc, wc), (hc, wc)]


def frame_bytes(H, W, chroma, depth):
    return sum(h * w for h, w in plane_shapes(H, W, chroma)) * (2 if depth > 8 else 1)


def planes(frame, H, W, chroma, depth):
    """the planes of one payload (a uint8 array of frame_bytes) as int64 arrays, every stored value above top read as top"""
    frame = np.ascontiguousarray(frame, dtype=np.uint8).reshape(-1)
    assert frame.size == frame_bytes(H, W, chroma, depth), (frame.size, frame_bytes(H, W, chroma, depth))
    v = (frame.view("<u2") if depth > 8 else frame).astype(np.int64)
    v = np.minimum(v, top(depth))
    out, lo = [], 0
    for h, w in plane_shapes(H, W, chroma):
        out.append(v[lo:lo + h * w].reshape(h, w))
        lo += h * w
    return out


def payload(plane_list, depth):
    """the inverse of planes(): integer planes -> the payload bytes (values are stored as they are, also above top)"""
    v = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in plane_list])
    return v.astype("<u2").view(np.uint8).copy() if depth > 8 else v.astype(np.uint8)


def ssim_plane(pa, pb, depth, dtype=np.float64):
    """mean SSIM of one plane pair on the [0,1] scale v / top; NaN under 11 samples on a side.  dtype float64: the restatement
    (metrics_images.ssim_f64).  dtype float32: the same definition evaluated in fp32 numpy (one division, fp32 maps, the mean of the map in
    float64) -- its distance from float64 is the unit D of the device test's bar at depths without a golden file."""
    h, w = pa.shape
    if h < 11 or w < 11:
        return float("nan")
    if dtype == np.float64:
        return mi.ssim_f64((pa / float(top(depth)))[None], (pb / float(top(depth)))[None])
    t = np.float32(top(depth))
    a, b = pa.astype(np.float32) / t, pb.astype(np.float32) / t
    g = mi.gaussian_window(np.float32)
    f = lambda x: mi._filter_valid(x, g)
    mu1, mu2 = f(a), f(b)
    s11, s22, s12 = f(a * a) - mu1 * mu1, f(b * b) - mu2 * mu2, f(a * b) - mu1 * mu2
    C1, C2 = np.float32(0.01) * np.float32(0.01), np.float32(0.03) * np.float32(0.03)
    m = ((np.float32(2) * mu1 * mu2 + C1) * (np.float32(2) * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    assert m.dtype == np.float32
    return float(m.astype(np.float64).mean())


def words(a, b, H, W, chroma, depth, prev=None, dtype=np.float64):
    """a, b: (B, frame_bytes) uint8; prev: None or (a_prev, b_prev), one payload each.  Returns (sse, dt, ssim, count): (B, 3) int64, int64,
    float64, int64 -- the four words of every plane.  A plane the format does not have: 0, 0, NaN, 0."""
    a, b = np.asarray(a), np.asarray(b)
    B = a.shape[0]
    sse, dt, count = (np.zeros((B, 3), dtype=np.int64) for _ in range(3))
    ssim = np.full((B, 3), np.nan)
    before = None if prev is None else (planes(prev[0], H, W, chroma, depth), planes(prev[1], H, W, chroma, depth))
    for k in range(B):
        pa, pb = planes(a[k], H, W, chroma, depth), planes(b[k], H, W, chroma, depth)
        for p in range(len(pa)):
            d = pa[p] - pb[p]
            sse[k, p] = int((d * d).sum())
            count[k, p] = d.size
            ssim[k, p] = ssim_plane(pa[p], pb[p], depth, dtype)
            if before is not None:
                dt[k, p] = int(np.abs((pa[p] - before[0][p]) - (pb[p] - before[1][p])).sum())
        before = (pa, pb)
    return sse, dt, ssim, count


def words_loops(a, b, H, W, chroma, depth, prev=None):
    """the same by a plain double loop over samples and windows, in Python floats: what the vectorised restatement is tested against"""
    t = float(top(depth))
    g = [math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)]
    g = [v / sum(g) for v in g]
    B = len(a)
    sse, dt, count = ([[0] * 3 for _ in range(B)] for _ in range(3))
    ssim = [[float("nan")] * 3 for _ in range(B)]
    before = None if prev is None else (planes(prev[0], H, W, chroma, depth), planes(prev[1], H, W, chroma, depth))
    for k in range(B):
        pa, pb = planes(a[k], H, W, chroma, depth), planes(b[k], H, W, chroma, depth)
        for p in range(len(pa)):
            h, w = pa[p].shape
            A, Bp = pa[p].tolist(), pb[p].tolist()
            for y in range(h):
                for x in range(w):
                    sse[k][p] += (A[y][x] - Bp[y][x]) ** 2
                    if before is not None:
                        dt[k][p] += abs((A[y][x] - int(before[0][p][y, x])) - (Bp[y][x] - int(before[1][p][y, x])))
            count[k][p] = h * w
            if h >= 11 and w >= 11:
                total = 0.0
                for y in range(h - 10):
                    for x in range(w - 10):
                        m1 = m2 = e11 = e22 = e12 = 0.0
                        for j in range(11):
                            for i in range(11):
                                wgt = g[j] * g[i]
                                u, v = A[y + j][x + i] / t, Bp[y + j][x + i] / t
                                m1 += wgt * u
                                m2 += wgt * v
                                e11 += wgt * u * u
                                e22 += wgt * v * v
                                e12 += wgt * u * v
                        s11, s22, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
                        total += ((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 * m1 + m2 * m2 + 1e-4) * (s11 + s22 + 9e-4))
                ssim[k][p] = total / ((h - 10) * (w - 10))
        before = (pa, pb)
    return sse, dt, ssim, count


# ---- seeded frame pairs -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair(H, W, chroma, depth, B, seed, kind="noisy"):
    """(a, b): two read-only (B, frame_bytes) uint8 arrays.  b: a 'clear' stream (blocks of 8 plus fine noise, drifting from frame to frame);
    a: b under a veil with less contrast and noise of its own.  kinds: noisy; one_sample (a = b but for one luma sample of the last frame);
    equal (a = b); extremes (a all top, b all 0); over_top (noisy, with some stored values above top -- only below 16 bits)"""
    rs = np.random.RandomState(seed)
    t = top(depth)
    a, b = [], []
    for k in range(B):
        pa, pb = [], []
        for h, w in plane_shapes(H, W, chroma):
            coarse = rs.randint(0, t + 1, (-(-h // 8), -(-w // 8))).astype(np.int64)
            clear = np.clip(np.kron(coarse, np.ones((8, 8), dtype=np.int64))[:h, :w] + rs.randint(-(t // 20) - 1, t // 20 + 2, (h, w)) + k * (t // 64), 0, t)
            hazy = np.clip(clear * 3 // 4 + t // 6 + rs.randint(-(t // 40) - 1, t // 40 + 2, (h, w)), 0, t)
            if kind == "extremes":
                clear, hazy = np.zeros_like(clear), np.full_like(clear, t)
            if kind in ("equal", "one_sample"):
                hazy = clear.copy()
                if kind == "one_sample" and k == B - 1 and not pa:
                    hazy[h // 2, w // 3] = (clear[h // 2, w // 3] + t // 2) % (t + 1)
            if kind == "over_top":
                assert depth < 16 and depth > 8
                over = rs.randint(0, 4, (h, w)) == 0
                clear = np.where(over & (clear > t // 2), clear + (65535 - t), clear)          # read as top
                hazy = np.where(rs.randint(0, 5, (h, w)) == 0, 65535, hazy)
            pa.append(hazy)
            pb.append(clear)
        a.append(payload(pa, depth))
        b.append(payload(pb, depth))
    a, b = np.stack(a), np.stack(b)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def y4m_payloads(data, H, W, chroma, depth):
    """(header line, (n, frame_bytes) uint8) of the bytes of a y4m file whose frame lines are plain `FRAME`"""
    nl = data.index(b"\n") + 1
    nb = frame_bytes(H, W, chroma, depth)
    rest = data[nl:]
    assert len(rest) % (6 + nb) == 0, (len(rest), nb)
    n = len(rest) // (6 + nb)
    rows = np.frombuffer(rest, dtype=np.uint8).reshape(n, 6 + nb)
    assert all(bytes(r[:6]) == b"FRAME\n" for r in rows)
    return data[:nl], np.ascontiguousarray(rows[:, 6:])
