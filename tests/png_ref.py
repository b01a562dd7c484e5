"""numpy restatement of the device PNG encoder's format (cfen_vit_dehazing_amd/png.py, csrc/k_png.hip): `stream(img)` gives the exact zlib stream
the kernels write for an (H,W,3) uint8 image -- same candidate tables (png.tables()), same filter choice and tie rule, same block choice, same
bit packing.  Written for clarity, not speed; nothing here shares code with the kernels.  Also the image cases of test_png_host.py / test_hip_png.py."""
import zlib

import numpy as np

import metrics_images
from cfen_vit_dehazing_amd import png


def filtered_scanlines(img):
    """(H, 1 + 3W) uint8: filter type byte + filtered bytes, the type with the smallest sum of |signed residual| per row, ties to the lowest"""
    H, W, _ = img.shape
    x = img.reshape(H, 3 * W).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]                       # left
    b = np.zeros_like(x)
    b[1:] = x[:-1]                             # up (zeros above row 0)
    c = np.zeros_like(x)
    c[1:, 3:] = x[:-1, :-3]                    # up-left
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cand = np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255          # (5, H, 3W)
    score = np.where(cand < 128, cand, 256 - cand).sum(axis=2)                      # (5, H)
    ftype = np.argmin(score, axis=0)                                                # the first minimum: the lowest type
    out = np.empty((H, 3 * W + 1), dtype=np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = cand[ftype, np.arange(H)]
    return out


def _pack(codes, lengths, first_bit):
    """bits of the (already bit-reversed) codes laid LSB first from bit `first_bit` on: (uint8 bit array from bit 0, zeros before first_bit)"""
    ends = first_bit + np.cumsum(lengths)
    bits = np.zeros(int(ends[-1]) if len(ends) else first_bit, dtype=np.uint8)
    starts = ends - lengths
    for k in range(int(lengths.max())):
        m = lengths > k
        bits[starts[m] + k] = (codes[m] >> k) & 1
    return bits


def strip_block(data):
    """one strip's bytes: (its deflate block + the empty stored block after it, index of the table used or -1 for stored)"""
    n = len(data)
    hist = np.bincount(data, minlength=257).astype(np.int64)
    hist[256] = 1
    tabs = png.tables()
    costs = [t.header_bits + int(hist @ np.asarray(t.lengths, dtype=np.int64)) for t in tabs]
    k = int(np.argmin(costs))                                      # the first minimum
    if costs[k] >= 8 * n + 40:
        return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + data.tobytes() + b"\x00\x00\x00\xff\xff", -1
    t = tabs[k]
    syms = np.concatenate([data.astype(np.int64), [256]])
    body = _pack(np.asarray(t.codes, dtype=np.int64)[syms], np.asarray(t.lengths, dtype=np.int64)[syms], t.header_bits)
    header = np.unpackbits(np.asarray(t.header_words, dtype="<u4").view(np.uint8), bitorder="little")[:t.header_bits]
    body[:t.header_bits] = header
    assert len(body) == costs[k]
    nbytes = (len(body) + 3 + 7) // 8                               # the 3 header bits of the empty stored block, then pad
    bits = np.zeros(nbytes * 8, dtype=np.uint8)
    bits[:len(body)] = body
    return np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff", k


def stream(img, blocks=None):
    """the zlib stream of an (H,W,3) uint8 image; `blocks`, if a list, receives the table index of every strip"""
    H, W, _ = img.shape
    R, S, rowb, _, _ = png.geometry(H, W)
    lines = filtered_scanlines(img)
    out = [b"\x78\x01"]
    for s in range(S):
        blk, k = strip_block(lines[s * R:(s + 1) * R].reshape(-1))
        out.append(blk)
        if blocks is not None:
            blocks.append(k)
    out.append(b"\x01\x00\x00\xff\xff")
    out.append((zlib.adler32(lines.tobytes()) & 0xFFFFFFFF).to_bytes(4, "big"))
    return b"".join(out)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def ramp(H, W):
    """value = (x + y + channel) mod 256: Sub leaves residual 1, Up leaves residual 1"""
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
    return _u8((x + y + c) & 255)


def noise(H, W, seed):
    return _u8(np.random.RandomState(seed).randint(0, 256, (H, W, 3)))


def smooth(H, W, seed):
    """image-like: a coarse random field enlarged, plus fine noise (integer arithmetic only)"""
    rs = np.random.RandomState(seed)
    coarse = rs.randint(0, 256, (-(-H // 16), -(-W // 16), 3)).astype(np.int64)
    big = np.kron(coarse, np.ones((16, 16, 1), dtype=np.int64))[:H, :W]
    return _u8(np.clip(big + rs.randint(-3, 4, (H, W, 3)), 0, 255))


# name -> (H,W,3) uint8.  W = 10922 gives a 32767-byte scanline (R = 1); 100 x 300 has R = 36, so a last strip of 28 rows; 700 x 20 has R = 537
SMALL_CASES = {
    "constant": lambda: np.full((40, 56, 3), 77, dtype=np.uint8),
    "ramp": lambda: ramp(96, 160),
    "noise": lambda: noise(64, 80, 1),
    "1x1": lambda: noise(1, 1, 2),
    "1xW": lambda: smooth(1, 333, 3),
    "Hx1": lambda: smooth(257, 1, 4),
    "R1_wide": lambda: smooth(3, 10922, 5),
    "short_last_strip": lambda: smooth(100, 300, 6),
    "tall_narrow": lambda: smooth(700, 20, 7),
    "metrics_37x53": lambda: metrics_images.pair("37x53")[0][0],
    "metrics_64x64_clear": lambda: metrics_images.pair("64x64")[1][0],
    "metrics_480x640": lambda: metrics_images.pair("480x640")[0][0],
    "metrics_black_white": lambda: metrics_images.pair("black_white_64x64")[1][0],
}
