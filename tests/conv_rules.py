"""The size rules of csrc/k_conv.hip, restated on the host (no GPU, no library): which k_conv instantiation launch_conv picks for a problem,
and how k_chan_stats / grid_img cut an image.  tests/test_conv_rules_host.py holds the restatement to the source (the switch arms it parses
and the constants it reads there); tests/test_hip_conv_geometry.py uses it to say which instantiation each of its cases runs, and a
kernel-trace of that file ties both to the library.

An instantiation is written  ("plain", TN, TM)  for launch_conv_t<T, TN, TM>,  ("wl", TN, TM, NW)  for launch_conv_wl_t<T, TN, TM, NW>
(weights staged in LDS, NW waves per workgroup) and  ("wl_up", TN, TM, NW)  for its UP = true form (source 1 interpolated x4 in LDS)."""

# launch_conv
SHRINK0_PX = 1 << 20          # px >= this: the full wave tile
SHRINK1_PX = 1 << 18          # px >= this: TM halved once; below: twice
FAT_BYTES = 16 * 1024         # staged matrices from this size on run 8-wave workgroups
WLDS_KB = {1: 60, 2: 150}     # "conv.wlds" -> largest staged matrix
WLDS_SHIPPED, WLDS_MAXLOG_SHIPPED = 2, 40
# k_chan_stats / grid_img
ST_CHUNKS = 64
STATS_U = 4                   # pixels per thread and pass
GRID_IMG_VECS, GRID_IMG_CAP = 2048, 128


def esize(dtype):
    """bytes per element; dtype: a torch dtype or its name"""
    name = str(dtype).replace("torch.", "")
    return {"float16": 2, "float32": 4}[name]


def kc(dtype):
    """K elements per MFMA chunk (Kpad is a multiple of it)"""
    return 32 if esize(dtype) == 2 else 16


def epl(dtype):
    """elements per 16-byte vector"""
    return 16 // esize(dtype)


def round_up(v, m):
    return (v + m - 1) // m * m


def kpad(dtype, cin_pad, k=3, nsrc=1, transpose=False):
    """Kpad of the packed weight (packing.pack_conv_weight / pack_convT_weight): taps * padded input channels, rounded up to the MFMA chunk"""
    taps = 4 if transpose else k * k * nsrc
    return round_up(taps * cin_pad, kc(dtype))


def conv_wl_pitch(dtype, Kpad):
    """bytes per LDS weight row: the row rounded up to 32 (mod 64)"""
    row = Kpad * esize(dtype)
    m = row & 63
    return row + (32 - m if m <= 32 else 96 - m)


def wl_bytes(dtype, Cout_pad, Kpad):
    return Cout_pad * conv_wl_pitch(dtype, Kpad)


def conv_px(ng, B, Hb, Wb, nphase):
    return ng * B * Hb * Wb * nphase


def shrink_of(px):
    return 0 if px >= SHRINK0_PX else 1 if px >= SHRINK1_PX else 2


def launch_conv(dtype, ng, B, Hb, Wb, nphase, Cout_pad, Kpad, wlds=WLDS_SHIPPED, wlds_maxlog=WLDS_MAXLOG_SHIPPED, up4=False):
    """the instantiation launch_conv<T> runs; ValueError where it refuses the problem"""
    px = conv_px(ng, B, Hb, Wb, nphase)
    shrink = shrink_of(px)
    wbytes = wl_bytes(dtype, Cout_pad, Kpad)
    fat = wbytes >= FAT_BYTES
    tn = Cout_pad // 16
    staged = {2: (2, 2, 8) if fat else (2, 1, 4) if shrink >= 2 else (2, 2, 4),
              3: (3, 2, 8) if fat else (3, 1, 4) if shrink >= 2 else (3, 2, 4),
              4: (4, 1, 8), 6: (6, 1, 8)}
    if up4:
        if esize(dtype) != 2 or tn not in staged:
            raise ValueError("conv (x4 source): fp16 and 32 / 48 / 64 / 96 output channels only")
        return ("wl_up",) + staged[tn]
    if wlds > 0 and wbytes <= WLDS_KB[2 if wlds > 1 else 1] * 1024 and px < (1 << wlds_maxlog) and tn in staged:
        return ("wl",) + staged[tn]
    plain = {1: (1, 2), 2: (2, 1) if shrink >= 2 else (2, 2), 3: (3, 1) if shrink >= 2 else (3, 2) if shrink == 1 else (3, 4),
             4: (4, 1) if shrink >= 1 else (4, 2), 6: (6, 1) if shrink >= 1 else (6, 2), 8: (8, 1)}
    if tn not in plain or Cout_pad % 16:
        raise ValueError("conv: Cout_pad=%d unsupported (16,32,48,64,96,128)" % Cout_pad)
    return ("plain",) + plain[tn]


def conv_problem(dtype, B, Hout, Wout, cin, cout, k=3, nsrc=1, transpose=False, wlds=WLDS_SHIPPED, ng=1):
    """launch_conv's choice for a layer as ops.conv2d describes it (one source of `cin` channels per tap, padded to 8; a transposed
    convolution is four phases over its INPUT grid, so pass the input's H and W)"""
    return launch_conv(dtype, ng, B, Hout, Wout, 4 if transpose else 1, round_up(cout, 16), kpad(dtype, round_up(cin, 8), k, nsrc, transpose), wlds)


def pixels_per_wave(inst):
    """output pixels of one wave of the instantiation: TM tiles of 16"""
    return inst[2] * 16


# ---------------------------------------------------------------------------------------------------
def chan_stats_plan(dtype, HW, C):
    """how k_chan_stats walks one image of HW pixels and C channels: a dict of
    per          pixels per chunk (ST_CHUNKS chunks; the last may be short, trailing ones empty)
    lanes        threads sharing one channel vector (256 // cv; the threads past lanes * cv idle)
    pass_pixels  pixels one pass of the loop covers (STATS_U * lanes)
    passes       passes over a full chunk
    last_pixels  pixels of the last non-empty chunk
    last_passes  passes over it
    ragged       pixels of a full chunk's last pass (pass_pixels: the pass is whole)
    empty        chunks with no pixel at all"""
    cv = C // epl(dtype)
    lanes = 256 // cv
    per = (HW + ST_CHUNKS - 1) // ST_CHUNKS
    used = (HW + per - 1) // per
    last = HW - (used - 1) * per
    pp = STATS_U * lanes
    ceil = lambda a, b: (a + b - 1) // b
    return dict(per=per, lanes=lanes, idle=256 - lanes * cv, pass_pixels=pp, passes=ceil(per, pp), last_pixels=last, last_passes=ceil(last, pp),
                ragged=per - (ceil(per, pp) - 1) * pp, empty=ST_CHUNKS - used)


def grid_img(dtype, HW, C):
    """blocks per image of the normalise / gate pass"""
    nvec = HW * (C // epl(dtype))
    g = (nvec + GRID_IMG_VECS - 1) // GRID_IMG_VECS
    return max(1, min(GRID_IMG_CAP, g))
