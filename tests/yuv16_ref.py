"""numpy restatement of the deep (9 to 16 bits per sample) YCbCr <-> float RGB conversion of include/cfen_yuv16.h, and a builder of deep
YUV4MPEG2 bytes.

Samples are unsigned 16-bit little-endian; all sums are int64, `>>` is an arithmetic shift; the floats are float32, divided and rounded by numpy's
IEEE arithmetic.  The 2^-20 tables are written out here as known answers (they were computed on the CPU); tests/test_yuv16_host.py holds
cfen_vit_dehazing_amd.yuv.tables(shift=20) to them.  The chroma geometry and both resampling rules are those of tests/yuv_ref.py (integer rules on
the sample values, whatever their depth) and are taken from there; the *_loops forms of that file serve the double-loop test."""
import numpy as np

import yuv_ref

CHROMAS = yuv_ref.CHROMAS
DEPTHS = (9, 10, 12, 14, 16)
TABLES = {            # (matrix, full_range): (forward, inverse), units of 2^-20
    ("bt601", False): ([[269262, 528618, 102662], [-155423, -305128, 460551], [460551, -385654, -74897]], [[1220945, 0, 1673555], [1220945, -410793, -852458], [1220945, 2115221, 0]]),
    ("bt601", True): ([[313524, 615514, 119538], [-176932, -347356, 524288], [524288, -439026, -85262]], [[1048576, 0, 1470104], [1048576, -360853, -748826], [1048576, 1858077, 0]]),
    ("bt709", False): ([[191455, 644068, 65019], [-105533, -355018, 460551], [460551, -418321, -42230]], [[1220945, 0, 1879825], [1220945, -223607, -558796], [1220945, 2215014, 0]]),
    ("bt709", True): ([[222927, 749942, 75707], [-120138, -404150, 524288], [524288, -476214, -48074]], [[1048576, 0, 1651297], [1048576, -196424, -490864], [1048576, 1945738, 0]]),
}
HALF = 1 << 19


def table(matrix, full_range):
    f, i = TABLES[(matrix, bool(full_range))]
    return np.array(f, dtype=np.int64), np.array(i, dtype=np.int64)


def levels(depth, full_range):
    """(oy, peak, centre, top)"""
    s = depth - 8
    top = (1 << depth) - 1
    return (0 if full_range else 16 << s), (top if full_range else 255 << s), 1 << (depth - 1), top


chroma_shape = yuv_ref.chroma_shape


def frame_samples(H, W, chroma):
    return yuv_ref.frame_bytes(H, W, chroma)


def frame_bytes(H, W, chroma):
    return 2 * frame_samples(H, W, chroma)


def samples(frame):
    """the uint16 samples of one frame's payload: bytes, a uint8 array or a uint16 array"""
    if isinstance(frame, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(frame), dtype="<u2")
    frame = np.asarray(frame)
    if frame.dtype == np.uint8:
        return np.frombuffer(frame.reshape(-1).tobytes(), dtype="<u2")
    return frame.reshape(-1).astype(np.uint16)


def payload(sample_values):
    """uint16 sample values -> the payload as a 1-D uint8 array (little endian)"""
    return np.frombuffer(np.asarray(sample_values).reshape(-1).astype("<u2").tobytes(), dtype=np.uint8)


def split(frame, H, W, chroma):
    """(Y, Cb, Cr) planes of one frame as uint16 arrays (Cb = Cr = None for mono)"""
    v = samples(frame)
    assert v.size == frame_samples(H, W, chroma)
    hc, wc = chroma_shape(H, W, chroma)
    y = v[:H * W].reshape(H, W)
    if chroma == "mono":
        return y, None, None
    return y, v[H * W:H * W + hc * wc].reshape(hc, wc), v[H * W + hc * wc:].reshape(hc, wc)


# ---- the pointwise formulas ------------------------------------------------------------------------------------------------------------
def inverse_pixels(ycc, inv, depth, full_range):
    """(..., 3) YCbCr sample values (already limited to top) -> (..., 3) integer RGB q in 0 .. peak, int64"""
    oy, peak, c, _ = levels(depth, full_range)
    ycc = np.asarray(ycc).astype(np.int64)
    y, cb, cr = ycc[..., 0] - oy, ycc[..., 1] - c, ycc[..., 2] - c
    out = np.empty(ycc.shape, dtype=np.int64)
    for k in range(3):
        out[..., k] = np.clip((inv[k, 0] * y + inv[k, 1] * cb + inv[k, 2] * cr + HALF) >> 20, 0, peak)
    return out


def forward_pixels(q, fwd, depth, full_range):
    """(..., 3) integer RGB q in 0 .. peak -> (..., 3) YCbCr values d in 0 .. top, int64"""
    oy, _, c, top = levels(depth, full_range)
    q = np.asarray(q).astype(np.int64)
    out = np.empty(q.shape, dtype=np.int64)
    for k, o in enumerate((oy, c, c)):
        out[..., k] = np.clip((fwd[k, 0] * q[..., 0] + fwd[k, 1] * q[..., 1] + fwd[k, 2] * q[..., 2] + (o << 20) + HALF) >> 20, 0, top)
    return out


def to_float(q, peak):
    """(float)(2 q - peak) / (float)peak: one correctly rounded float32 division"""
    return ((2 * np.asarray(q, dtype=np.int64) - peak).astype(np.float32) / np.float32(peak)).astype(np.float32)


def quantise(x, peak):
    """float32 in [-1, 1] -> q in 0 .. peak: t = x * 0.5 + 0.5 in float32, clamped to [0, 1] with NaN -> 0, rint(t * peak) half to even"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = x * np.float32(0.5) + np.float32(0.5)
        t = np.where(t >= 0, np.minimum(t, np.float32(1.0)), np.float32(0.0)).astype(np.float32)       # NaN fails t >= 0
        return np.rint(t * np.float32(peak)).astype(np.int64)


# ---- whole frames ----------------------------------------------------------------------------------------------------------------------
def yuv_to_rgb(frame, H, W, chroma, depth, matrix="bt601", full_range=False, up=yuv_ref.upsample):
    """one frame's payload -> (3, H, W) float32"""
    _, inv = table(matrix, full_range)
    _, peak, c, top = levels(depth, full_range)
    y, cb, cr = split(frame, H, W, chroma)
    ycc = np.empty((H, W, 3), dtype=np.int64)
    ycc[..., 0] = np.minimum(y.astype(np.int64), top)
    if chroma == "mono":
        ycc[..., 1:] = c
    else:
        ycc[..., 1] = up(np.minimum(cb.astype(np.int64), top), H, W, chroma)
        ycc[..., 2] = up(np.minimum(cr.astype(np.int64), top), H, W, chroma)
    return np.ascontiguousarray(to_float(inverse_pixels(ycc, inv, depth, full_range), peak).transpose(2, 0, 1))


def rgb_to_yuv(rgb, chroma, depth, matrix="bt601", full_range=False, down=yuv_ref.downsample):
    """(3, H, W) float32 -> the frame's payload, a 1-D uint8 array"""
    fwd, _ = table(matrix, full_range)
    _, peak, _, _ = levels(depth, full_range)
    q = quantise(np.asarray(rgb, dtype=np.float32).transpose(1, 2, 0), peak)
    d = forward_pixels(q, fwd, depth, full_range)
    planes = [d[..., 0]]
    if chroma != "mono":
        planes += [down(d[..., 1], chroma), down(d[..., 2], chroma)]
    return payload(np.concatenate([p.reshape(-1) for p in planes]))


# ---- YUV4MPEG2 bytes -------------------------------------------------------------------------------------------------------------------
def ctag(chroma, depth):
    """the C tag's value for a deep stream: 420p10, 422p12, 444p16, mono12, ... (4:2:0 is the co-sited 420mpeg2 geometry)"""
    return "mono%d" % depth if chroma == "mono" else "%sp%d" % ({"420mpeg2": "420"}.get(chroma, chroma), depth)


def y4m_header(W, H, chroma, depth, tags=("F25:1", "Ip", "A1:1"), extra=()):
    return (" ".join(["YUV4MPEG2", "W%d" % W, "H%d" % H] + list(tags) + ["C" + ctag(chroma, depth)] + list(extra)) + "\n").encode()


def y4m_bytes(frames, W, H, chroma, depth, header=None, frame_line=b"FRAME\n"):
    out = [header if header is not None else y4m_header(W, H, chroma, depth)]
    for f in frames:
        f = bytes(f) if isinstance(f, (bytes, bytearray)) else np.asarray(f, dtype=np.uint8).reshape(-1).tobytes()
        assert len(f) == frame_bytes(H, W, chroma)
        out += [frame_line, f]
    return b"".join(out)


def y4m_frames(data, H, W, chroma):
    """(header line with its newline, [payload bytes of every frame as uint8 arrays]) of a stream built with plain FRAME lines"""
    nl = data.index(b"\n")
    header, body, n = data[:nl + 1], data[nl + 1:], frame_bytes(H, W, chroma)
    frames = []
    while body:
        assert body[:6] == b"FRAME\n", body[:16]
        assert len(body) >= 6 + n
        frames.append(np.frombuffer(body[6:6 + n], dtype=np.uint8))
        body = body[6 + n:]
    return header, frames
