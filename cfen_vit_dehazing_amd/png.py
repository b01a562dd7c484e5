"""PNG encoding on the device (`test.py --gpu_png`; csrc/k_png.hip; include/cfen_hip.h, cfen_png_deflate).

The file is an 8-bit RGB, non-interlaced PNG: signature, IHDR, ONE IDAT, IEND.  The IDAT payload is one zlib stream made by the kernels:

    78 01 | per strip of rows: one non-final deflate block + an empty non-final stored block | 01 00 00 FF FF | Adler-32 (big-endian)

  strips     R = max(1, 32768 // (3 W + 1)) rows each (the last may be shorter): a strip's filtered scanlines (filter byte + 3 W bytes a row) are
             at most 32768 bytes.  An image whose scanline is longer than that is refused (RowTooLong; `encode` writes it with PIL).
  filtering  per row the type (None, Sub, Up, Average, Paeth) with the smallest sum of |signed residual| (libpng's heuristic), ties to the
             lowest type; the row above row 0 is zeros.
  coding     literals only (no LZ77): the cheapest of the K = 16 fixed candidate tables below as a dynamic-Huffman block, or a stored block
             when no table is strictly smaller than 8 n + 40 bits.  The empty stored block after it (000, pad to a byte, 00 00 FF FF: zlib's
             sync flush) byte-aligns the next strip, so strips are coded independently.

The candidate tables are made here, once, on the host: the kernel only picks one.  `tests/png_ref.py` restates the format in numpy from the same
tables and gives the same bytes.  The host is left with the container: one CRC-32 and one write per image (`assemble`)."""
import math
import struct
import threading
import zlib

import numpy as np

MAX_STRIP = 32768                 # filtered bytes per strip, and the longest scanline (3 W + 1) the encoder takes
N_SYMBOLS = 257                   # literals 0..255 + end of block
MAX_BITS = 15
TABLE_WORDS = 384                 # uint32 words per table in the blob handed to the kernel (include/cfen_hip.h)
TABLE_HEADER_WORDS = 63           # words 1..63: the block header, packed LSB first; word 0: its length in bits
TABLE_CODES_AT = 64               # words 64..320: (length << 16) | bit-reversed code of symbol 0..256
# mean |residual| of the two-sided geometric distribution a table is built for: 16 values spaced geometrically (ratio (64 / 0.72)^(1/15)) from
# 0.72 -- the tightest whose Huffman code still gives residuals 0, +1 and -1 at most 3 bits -- to 64 (past that a stored block wins)
SCALES = tuple(0.72 * (64.0 / 0.72) ** (k / 15.0) for k in range(16))
_WEIGHT_ONE = 1 << 24             # integer weight of probability 1; every symbol gets at least 1
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


class RowTooLong(ValueError):
    """the scanline of this image (1 + 3 W bytes) does not fit a strip"""


# ---------------------------------------------------------------------------------------------------------------- geometry
def geometry(H, W):
    """(R rows per strip, S strips, scanline bytes, bytes per strip slot of the workspace, bytes per image of the output slab) -- the same
    arithmetic as cfen_png_workspace_bytes"""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("png: empty image %d x %d" % (H, W))
    rowb = 3 * W + 1
    if rowb > MAX_STRIP:
        raise RowTooLong("png: a scanline of %d bytes (width %d) is longer than the %d-byte strip of the device encoder" % (rowb, W, MAX_STRIP))
    R = max(1, MAX_STRIP // rowb)
    S = -(-H // R)
    strip_bytes = (min(R, H) * rowb + 16 + 15) // 16 * 16
    out_stride = (2 + H * rowb + 10 * S + 9 + 15) // 16 * 16       # header, every strip stored (n + 10), closing block, Adler-32
    return R, S, rowb, strip_bytes, out_stride


# ---------------------------------------------------------------------------------------------------------------- tables
def limited_lengths(weights, limit):
    """code lengths of a length-limited Huffman code (package-merge): positive integer weights -> lengths in 1..limit with Kraft sum exactly 1;
    weight 0 -> length 0 (symbol not coded).  Ties go to the lower symbol, so the result is the same everywhere."""
    used = [i for i, w in enumerate(weights) if w > 0]
    n = len(used)
    if n < 2 or n > (1 << limit):
        raise ValueError("limited_lengths: %d used symbols do not make a complete code of at most %d bits" % (n, limit))
    leaves = sorted((int(weights[i]), j) for j, i in enumerate(used))
    eye = np.eye(n, dtype=np.int32)
    leaf_items = [(w, eye[j]) for w, j in leaves]
    level = list(leaf_items)
    for _ in range(limit - 1):
        packages = [(level[2 * j][0] + level[2 * j + 1][0], level[2 * j][1] + level[2 * j + 1][1]) for j in range(len(level) // 2)]
        merged, a, b = [], 0, 0
        while a < n or b < len(packages):              # stable merge, a leaf before a package of the same weight
            if b >= len(packages) or (a < n and leaf_items[a][0] <= packages[b][0]):
                merged.append(leaf_items[a])
                a += 1
            else:
                merged.append(packages[b])
                b += 1
        level = merged
    counts = sum(item[1] for item in level[:2 * n - 2])
    out = [0] * len(weights)
    for j, i in enumerate(used):
        out[i] = int(counts[j])
    return out


def canonical_codes(lengths):
    """canonical Huffman codes (RFC 1951 3.2.2) of the given lengths, most significant bit first"""
    codes, code = [0] * len(lengths), 0
    for bits in range(1, max(lengths) + 1):
        for s, l in enumerate(lengths):
            if l == bits:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def bit_reverse(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


class _Bits:
    """deflate's bit order: values go in from the least significant bit, Huffman codes arrive already reversed"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):
        self.acc |= int(value) << self.n
        self.n += nbits

    def words(self, count):
        if self.n > 32 * count:
            raise ValueError("block header of %d bits does not fit %d words" % (self.n, count))
        return [(self.acc >> (32 * i)) & 0xFFFFFFFF for i in range(count)]


def symbol_weights(scale):
    """integer weights of the 257 symbols for a two-sided geometric residual with mean |r| parameter `scale`: theta^min(v, 256 - v); the end-of-block
    symbol (once per strip) gets the floor weight"""
    theta = math.exp(-1.0 / scale)
    norm = (1.0 - theta) / (1.0 + theta)
    w = [max(1, int(norm * theta ** min(v, 256 - v) * _WEIGHT_ONE + 0.5)) for v in range(256)]
    return w + [1]


def _dynamic_header(lengths):
    """the bits of a non-final dynamic block up to its first symbol: BFINAL 0, BTYPE 2, HLIT 257, HDIST 1 with that one distance code of
    length 0 ("no distance codes", RFC 1951 3.2.7), the code-length code, the run-length coded lengths"""
    seq = list(lengths) + [0]
    runs, i = [], 0                                       # (code-length symbol, extra bits value, extra bits count)
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        i = j
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                runs.append((18, r - 11, 7))
                run -= r
            if run >= 3:
                runs.append((17, run - 3, 3))
                run = 0
            runs.extend([(0, 0, 0)] * run)
            continue
        runs.append((v, 0, 0))
        run -= 1
        while run >= 3:
            r = min(run, 6)
            runs.append((16, r - 3, 2))
            run -= r
        runs.extend([(v, 0, 0)] * run)
    freq = [0] * 19
    for s, _, _ in runs:
        freq[s] += 1
    cl_len = limited_lengths(freq, 7)
    cl_code = canonical_codes(cl_len)
    hclen = max(k for k in range(19) if cl_len[_CL_ORDER[k]]) + 1
    bits = _Bits()
    bits.put(0, 1)
    bits.put(2, 2)
    bits.put(N_SYMBOLS - 257, 5)
    bits.put(0, 5)
    bits.put(max(hclen, 4) - 4, 4)
    for k in range(max(hclen, 4)):
        bits.put(cl_len[_CL_ORDER[k]], 3)
    for s, extra, nextra in runs:
        bits.put(bit_reverse(cl_code[s], cl_len[s]), cl_len[s])
        bits.put(extra, nextra)
    return bits


class Table:
    """one candidate code: lengths[257], codes[257] (bit-reversed, ready for LSB-first packing), the block header as bits"""

    def __init__(self, scale):
        self.scale = scale
        self.lengths = limited_lengths(symbol_weights(scale), MAX_BITS)
        self.codes = [bit_reverse(c, l) for c, l in zip(canonical_codes(self.lengths), self.lengths)]
        header = _dynamic_header(self.lengths)
        self.header_bits = header.n
        self.header_words = header.words(TABLE_HEADER_WORDS)

    def blob(self):
        w = np.zeros(TABLE_WORDS, dtype=np.uint32)
        w[0] = self.header_bits
        w[1:1 + TABLE_HEADER_WORDS] = self.header_words
        w[TABLE_CODES_AT:TABLE_CODES_AT + N_SYMBOLS] = [(l << 16) | c for l, c in zip(self.lengths, self.codes)]
        return w


_tables = None
_tables_lock = threading.Lock()
_device_tables = {}


def tables():
    """the K candidate tables, tightest first (made once)"""
    global _tables
    with _tables_lock:
        if _tables is None:
            _tables = tuple(Table(s) for s in SCALES)
    return _tables


def table_blob():
    """(K, TABLE_WORDS) uint32: what cfen_png_deflate takes as `tables`"""
    return np.stack([t.blob() for t in tables()])


def device_tables(device):
    """the table blob on `device`, uploaded once per device"""
    import torch
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    with _tables_lock:
        t = _device_tables.get(device)
    if t is None:
        t = torch.from_numpy(table_blob().view(np.int32)).to(device)
        with _tables_lock:
            t = _device_tables.setdefault(device, t)
    return t


# ---------------------------------------------------------------------------------------------------------------- container
def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF)


def assemble(stream, H, W):
    """the PNG file around a finished zlib stream of the filtered scanlines of an H x W 8-bit RGB image (bytes, bytearray, memoryview or a uint8
    array): signature, IHDR, one IDAT, IEND"""
    return b"".join((_PNG_SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", int(W), int(H), 8, 2, 0, 0, 0)),
                     _chunk(b"IDAT", bytes(stream)), _chunk(b"IEND", b"")))


def _pil_bytes(arr):
    import io

    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


# ---------------------------------------------------------------------------------------------------------------- device encode
class Pending:
    """an encode in flight: `wait()` then `files()`.  slab / lengths are pinned host buffers the copy was queued into on the caller's stream"""

    def __init__(self, slab, lengths, event, H, W):
        self.slab, self.lengths, self.event, self.H, self.W = slab, lengths, event, H, W

    def wait(self):
        self.event.synchronize()
        return self

    def stream(self, i):
        """image i's zlib stream, a view of the pinned slab (valid until the buffers are reused)"""
        return self.slab[i, :int(self.lengths[i])].numpy()

    def files(self):
        self.wait()
        return [assemble(self.stream(i), self.H, self.W) for i in range(self.slab.shape[0])]


def encode_async(images_u8, slab=None, lengths=None):
    """queue the encode of a contiguous (B,H,W,3) uint8 CUDA tensor and the copy of its streams to pinned host memory on the current stream.
    slab (B, out_stride) uint8 / lengths (B,) int32: pinned host buffers to reuse (else allocated).  The copy is the whole fixed-stride slab."""
    import torch

    from . import ops
    if images_u8.dim() == 3:
        images_u8 = images_u8[None]
    B, H, W, _ = images_u8.shape
    dev_slab, dev_len = ops.png_deflate(images_u8)
    if slab is None:
        slab = torch.empty(dev_slab.shape, dtype=torch.uint8, pin_memory=True)
    if lengths is None:
        lengths = torch.empty(B, dtype=torch.int32, pin_memory=True)
    if tuple(slab.shape) != tuple(dev_slab.shape) or tuple(lengths.shape) != (B,):
        raise ValueError("encode_async: host buffers must be %s uint8 and (%d,) int32" % (tuple(dev_slab.shape), B))
    slab.copy_(dev_slab, non_blocking=True)
    lengths.copy_(dev_len, non_blocking=True)
    event = torch.cuda.Event()
    event.record()
    # the device buffers go back to the caching allocator here; it reuses them in stream order, after the copies above
    return Pending(slab, lengths, event, H, W)


def encode(images_u8):
    """PNG files (bytes) of a (B,H,W,3) or (H,W,3) uint8 CUDA tensor.  An image too wide for the device encoder (RowTooLong) is written by PIL."""
    if images_u8.dim() == 3:
        images_u8 = images_u8[None]
    try:
        geometry(images_u8.shape[1], images_u8.shape[2])
    except RowTooLong:
        return [_pil_bytes(a) for a in images_u8.cpu().numpy()]
    return encode_async(images_u8.contiguous()).files()


# ---------------------------------------------------------------------------------------------------------------- test.py --gpu_png
def visual_u8(batch):
    """one visual of a batch as the (B,H,W,3) uint8 CUDA tensor of util.tensor2im's bytes: uint8 images as they are, float (B,1|3,H,W) through the
    device pass the PIL path uses as well (ops.tensor2im_u8)"""
    import torch

    from . import ops
    if batch.dtype == torch.uint8:
        return batch.contiguous()
    return torch.stack([ops.tensor2im_u8(batch[b].float().contiguous()) for b in range(batch.shape[0])])


def write_stream(stream, H, W, path):
    """what a writer thread does with a finished stream: container, CRC-32, one write"""
    with open(path, "wb") as f:
        f.write(assemble(stream, H, W))


def save_images(image_dir, visuals, image_path):
    """util.visualizer.save_images with the encode on the device: `<stem>_<label>.png` per image and visual, the same pixels as the PIL path writes"""
    import ntpath
    import os
    for label, data in visuals.items():
        files = encode(visual_u8(data))
        for i, path in enumerate(image_path):
            name = os.path.splitext(ntpath.basename(path))[0]
            with open(os.path.join(image_dir, "%s_%s.png" % (name, label)), "wb") as f:
                f.write(files[i])


def check_options(opt):
    """--gpu_png against the options that configure the host encoder it replaces"""
    if not getattr(opt, "gpu_png", False):
        return
    if getattr(opt, "writer_procs", 0) > 0:
        raise ValueError("--gpu_png encodes on the device and leaves the writer threads one CRC and one write per image: --writer_procs %d would fork "
                         "encoder processes with nothing to encode; drop one of the two" % opt.writer_procs)
    if getattr(opt, "png_compress_level", -1) != -1:
        raise ValueError("--gpu_png does not go through zlib: --png_compress_level %d has no meaning for its Huffman-only streams; drop one of the two"
                         % opt.png_compress_level)
