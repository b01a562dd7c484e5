"""Integer YCbCr <-> RGB tables and the plane geometry of a YUV4MPEG2 frame (host only; include/cfen_yuv.h states the definition the
kernels of csrc/k_yuv.hip compute with these tables, tests/yuv_ref.py restates it in numpy).

All arithmetic downstream of the tables is integer, `>>` is an arithmetic shift:
    Y|Cb|Cr = clamp((row . (R, G, B) + (o << 14) + 8192) >> 14, 0, 255)         o = oy, 128, 128
    R|G|B   = clamp((row . (Y - oy, Cb - 128, Cr - 128) + 8192) >> 14, 0, 255)
"""
import numpy as np

SHIFT = 14
ONE = 1 << SHIFT
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}           # (Kr, Kb)
# the C values of a y4m header this project reads, and the `chroma` argument of the C functions (CFEN_YUV_* of include/cfen_yuv.h)
CHROMA = {"420jpeg": 0, "420mpeg2": 1, "422": 2, "444": 3, "mono": 4}
MAX_EDGE = 65536
MAX_BATCH = 65535
# deep samples (include/cfen_yuv16.h): the kernels take every depth of 9 .. 16 bits; DEPTHS are the ones a y4m header can name
DEEP_SHIFT = 20
MIN_DEPTH, MAX_DEPTH = 9, 16
DEPTHS = (9, 10, 12, 14, 16)


def _float_matrices(matrix, full_range):
    if matrix not in MATRICES:
        raise ValueError("yuv: matrix must be one of %s, got %r" % (sorted(MATRICES), matrix))
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (255.0, 255.0) if full_range else (219.0, 224.0)
    fwd = np.array([[kr, kg, kb],
                    [-0.5 * kr / (1 - kb), -0.5 * kg / (1 - kb), 0.5],
                    [0.5, -0.5 * kg / (1 - kr), -0.5 * kb / (1 - kr)]], dtype=np.float64)
    fwd[0] *= ys / 255.0
    fwd[1:] *= cs / 255.0
    sy, sc = 255.0 / ys, 255.0 / cs
    inv = np.array([[sy, 0.0, sc * 2 * (1 - kr)],
                    [sy, -sc * 2 * (1 - kb) * kb / kg, -sc * 2 * (1 - kr) * kr / kg],
                    [sy, sc * 2 * (1 - kb), 0.0]], dtype=np.float64)
    return fwd, inv, ys


def float_matrices(matrix, full_range):
    """(forward, inverse, oy) in float64: what the integer tables round; the offsets are (oy, 128, 128)"""
    fwd, inv, _ = _float_matrices(matrix, full_range)
    return fwd, inv, (0 if full_range else 16)


def tables(matrix="bt601", full_range=False, shift=SHIFT):
    """(forward, inverse, oy): two (3, 3) int32 tables in units of 2^-shift and the 8-bit luma offset (16 limited, 0 full).

    forward: rint(f * 2^shift), then every row sum is repaired on the entry of largest magnitude: the luma row sums to round(ys / 255 * 2^shift)
    (ys = 219 limited, 255 full), the chroma rows to 0, so R = G = B gives Cb = Cr = the centre exactly.  inverse: rint(f^-1 * 2^shift), no
    repair.  shift = 14 is the 8-bit route (include/cfen_yuv.h), shift = 20 the deep one (include/cfen_yuv16.h; its offsets are levels(depth))."""
    if shift not in (14, 20):
        raise ValueError("yuv: tables are in units of 2^-14 (8-bit) or 2^-20 (9 to 16 bits), got shift = %r" % (shift,))
    one = 1 << shift
    fwd, inv, ys = _float_matrices(matrix, bool(full_range))
    f = np.rint(fwd * one).astype(np.int64)
    want = (int(round(ys / 255.0 * one)), 0, 0)
    for r in range(3):
        k = int(np.argmax(np.abs(f[r])))
        f[r, k] += want[r] - int(f[r].sum())
    i = np.rint(inv * one).astype(np.int64)
    return f.astype(np.int32), i.astype(np.int32), (0 if full_range else 16)


def chroma_code(chroma):
    if chroma not in CHROMA:
        raise ValueError("yuv: chroma must be one of %s, got %r" % (list(CHROMA), chroma))
    return CHROMA[chroma]


def chroma_shape(H, W, chroma):
    """(Hc, Wc) of the Cb and Cr planes; (0, 0) for mono.  Odd sizes are legal: the last column / row of chroma covers one pixel."""
    code = chroma_code(chroma)
    if code == 4:
        return 0, 0
    if code == 3:
        return H, W
    return ((H + 1) >> 1 if code < 2 else H), (W + 1) >> 1


def frame_bytes(H, W, chroma, depth=8):
    """payload bytes of one frame: the planes Y, Cb, Cr back to back, as in the file (cfen_yuv_frame_bytes computes the same); two bytes per
    sample for a depth of 9 to 16 (cfen_yuv16_frame_bytes)"""
    hc, wc = chroma_shape(H, W, chroma)
    return (H * W + 2 * hc * wc) * (1 if check_depth(depth) == 8 else 2)


def check_depth(depth):
    if depth != 8 and not (isinstance(depth, int) and MIN_DEPTH <= depth <= MAX_DEPTH):
        raise ValueError("yuv: depth must be 8 or %d .. %d bits per sample, got %r" % (MIN_DEPTH, MAX_DEPTH, depth))
    return depth


def levels(depth, full_range):
    """(oy, peak, centre) of a depth of 9 .. 16 bits (include/cfen_yuv16.h): the luma offset 16 << (depth - 8) limited and 0 full, the RGB full
    scale 255 << (depth - 8) limited and 2^depth - 1 full, the chroma centre 1 << (depth - 1).  depth 8 gives (16 | 0, 255, 128)."""
    s = check_depth(depth) - 8
    return (0 if full_range else 16 << s), ((1 << depth) - 1 if full_range else 255 << s), 1 << (depth - 1)
