"""The conv / norm stack where the problem's SIZE and SHAPE pick the code: k_conv's wave tiles selected by the pixel count, every k_conv
instantiation on maps with H != W, k_chan_stats' multi-pass / short / empty chunks and grid_img's cap, patchify on a non-square map.

tests/conv_rules.py restates launch_conv's choice and the statistics' chunking; every case below names the instantiation it is there for
(`claim`), tests/test_conv_rules_host.py checks without a GPU that the claims are what the rule gives and that claims + excuses cover the
switch in csrc/k_conv.hip, and each GPU case asserts its claim again before it runs.

a. SIZE_CASES: the TM = 2 / TM = 4 tiles, reached only from 2^18 pixels on.  Two maps: 3 x 187 x 480 = 269,280 pixels (2^18 <= px < 2^20,
   no multiple of 256) and 5 x 211 x 1008 = 1,063,440 pixels (>= 2^20, 16 pixels left over after the last full wave of 64): H odd, H != W,
   W a multiple of 16 but not of 64, so a wave's run of pixels crosses row ends and image ends.  Reference: float64 unfold + matmul in
   plain torch on the device (the CPU needs ~10 s per map), held equal to the CPU's float64 F.conv2d on a corner crop of the last image.
b. GEOM_CASES: every instantiation a small map reaches at the shipped knobs, on 3 x 7 x 48 maps (stride 2 from 13 x 95, reflect 7x7 on
   5 rows, NCHW fp32 output, two and three sources with ActNorm + ReLU + two residuals, ConvTranspose2d on 5 x 16) in guard-band
   tensors, and a one-hot shift that must come out bit-exact.
c. STATS_CASES: InstanceNorm + ReLU and CFSM2G where a chunk takes several passes, the last chunk is short, chunks are empty, 256 / cv is
   not whole, and the apply grid is at its cap of 128 blocks.
d. patchify / unpatchify on 32 x 96.

Value-only mutations of csrc/k_conv.hip these cases were seen to catch on an MI355X while tests/test_hip_ops.py, test_hip_bounds.py and
test_hip_value_edges.py passed with all three in: tile j = 1 of the TM = 2 / 4 instantiations storing tile 0's values (every px2e18 / px2e20
case of a); res1 not added (the two- and three-source cases of b); k_chan_stats leaving out the last pass of a multi-pass chunk (every
case of c but hw40)."""
import collections
import math

import pytest
import torch
import torch.nn.functional as F

import cfen_oracle
import conv_rules
import value_edges_ref as ve
from cfen_vit_dehazing_amd import ops, packing
from guarded import check_bands, guarded_copy, guarded_empty
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from test_hip_ops import DTYPES, close, dev, perm_tokens, rnd, run_conv, tol

pytestmark = pytest.mark.gpu

F16, F32 = "float16", "float32"


def _name(dtype):
    return str(dtype).replace("torch.", "")


# ---- a. size-selected instantiations ------------------------------------------------------------------------------------------------------
MAPS = {"px2e18": (3, 187, 480), "px2e20": (5, 211, 1008), "small": (3, 7, 48)}      # (B, Hout, Wout)

# epi: "bias" = conv + bias at tol 4 (test_conv_plain's bar); "relu_res" = bias + ReLU + res0 at tol 6; "an_relu_res" = bias + ActNorm + ReLU + res0 at tol 6
SizeCase = collections.namedtuple("SizeCase", "id map cin cout k stride nsrc epi wlds claim")
SIZE_CASES = (
    # "conv.wlds" 0 on the first map
    SizeCase("plain_2x2", "px2e18", 8, 24, 3, 1, 1, "bias", 0, ("plain", 2, 2)),
    SizeCase("plain_3x2_stride2_relu_res", "px2e18", 8, 40, 3, 2, 1, "relu_res", 0, ("plain", 3, 2)),       # from 373 x 959
    # "conv.wlds" 0 on the second map
    SizeCase("plain_3x4_relu_res", "px2e20", 8, 40, 3, 1, 1, "relu_res", 0, ("plain", 3, 4)),
    SizeCase("plain_4x2_stride2", "px2e20", 8, 56, 3, 2, 1, "bias", 0, ("plain", 4, 2)),                    # from 421 x 2015
    SizeCase("plain_6x2", "px2e20", 8, 88, 3, 1, 1, "bias", 0, ("plain", 6, 2)),
    # shipped knobs on the first map: staged matrices below 16 KiB in both dtypes (3x3 over 8 channels: 7 / 11 KiB at 32 rows; the 48-row
    # matrix of a 3x3 is 16.5 KiB in fp32, so the 1x1 fuse conv over two maps of 24 channels: 7.5 / 10.5 KiB)
    SizeCase("staged_2x2x4_relu_res", "px2e18", 8, 24, 3, 1, 1, "relu_res", 2, ("wl", 2, 2, 4)),
    SizeCase("staged_3x2x4_two_sources_actnorm", "px2e18", 24, 40, 1, 1, 2, "an_relu_res", 2, ("wl", 3, 2, 4)),
    # TM = 1 without staged weights
    SizeCase("plain_3x1", "small", 8, 40, 3, 1, 1, "relu_res", 0, ("plain", 3, 1)),
    SizeCase("plain_4x1", "small", 8, 56, 3, 1, 1, "bias", 0, ("plain", 4, 1)),
)


def size_case_rule(c, dtype):
    """the instantiation conv_rules gives the case in `dtype`"""
    B, H, W = MAPS[c.map]
    return conv_rules.conv_problem(dtype, B, H, W, c.cin, c.cout, c.k, c.nsrc, wlds=c.wlds)


def _group_key(c):
    return (c.map, c.cin, c.k, c.stride, c.nsrc)


def _conv64_on_device(xs, w, k, stride, pad):
    """float64 convolution of the channel concat of xs as unfold + matmul, plain torch on the device"""
    x = torch.cat([t.to(dev()).double() for t in xs], 1)
    B, _, H, W = x.shape
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    cols = F.unfold(x, k, padding=pad, stride=stride)
    return (w.to(dev()).double().reshape(w.shape[0], -1) @ cols).view(B, w.shape[0], Ho, Wo)


def _corner_crop_equals_cpu(xs, w, k, stride, pad, ref):
    """the device reference against the CPU's float64 F.conv2d on the bottom-right corner of the last image (the crop's first output row and
    column see the cut instead of the map and are left out)"""
    x = torch.cat([t[-1:] for t in xs], 1).double()
    Hin, Win = x.shape[2:]
    r0, c0 = max(0, (Hin - 40) // stride * stride), max(0, (Win - 40) // stride * stride)
    got = F.conv2d(x[:, :, r0:, c0:], w.double(), stride=stride, padding=pad)[0, :, 1:, 1:]
    want = ref[-1, :, r0 // stride + 1:, c0 // stride + 1:].cpu()
    assert got.shape == want.shape and got.shape[1] >= 4 and got.shape[2] >= 4
    d = float((got - want).abs().max())
    assert d <= 1e-12, "float64 reference on the device differs from the CPU's on the corner crop: %.3e" % d


@pytest.fixture(scope="module")
def size_refs():
    """{(group, dtype): (xs, w, ref)}: the operands of a group of cases (one map, one kernel geometry) and their float64 convolution for the
    widest case, computed once; a case takes the first `cout` filters.  Freed with the module."""
    cache = {}
    yield cache
    cache.clear()
    torch.cuda.empty_cache()


def _size_group(cache, c, dtype):
    key = (_group_key(c), dtype)
    if key not in cache:
        B, Ho, Wo = MAPS[c.map]
        pad = c.k // 2
        Hin, Win = ((Ho, Wo) if c.stride == 1 else (2 * Ho - 1, 2 * Wo - 1))            # stride 2: an odd input (373 x 959, 421 x 2015)
        cout = max(o.cout for o in SIZE_CASES if _group_key(o) == _group_key(c))
        xs = [rnd((B, c.cin, Hin, Win), 1 + i, dtype) for i in range(c.nsrc)]
        w = rnd((cout, c.nsrc * c.cin, c.k, c.k), 7, dtype, 1 / math.sqrt(c.nsrc * c.cin * c.k * c.k))
        ref = _conv64_on_device(xs, w, c.k, c.stride, pad)
        assert tuple(ref.shape[2:]) == (Ho, Wo)
        _corner_crop_equals_cpu(xs, w, c.k, c.stride, pad, ref)
        cache[key] = (xs, w, ref)
    return cache[key]


def close_on_device(got, want, atol, what=""):
    """test_hip_ops.close for the big maps: the same assertion, the difference taken on the device (both sides are there already)"""
    d = float((got.double() - want).abs().max())
    assert d <= atol, "%s max-abs %.3e > %.1e" % (what, d, atol)
    return d


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", SIZE_CASES, ids=[c.id for c in SIZE_CASES])
def test_conv_size_selected_instantiation(c, dtype, size_refs):
    assert size_case_rule(c, dtype) == c.claim
    B, Ho, Wo = MAPS[c.map]
    px = B * Ho * Wo
    assert conv_rules.shrink_of(px) == {"px2e18": 1, "px2e20": 0, "small": 2}[c.map]
    if c.map == "px2e18":
        assert px % 256 != 0
    if c.map == "px2e20":
        assert px % 64 == 16                                     # the last wave of a TM = 4 tile holds one tile of 16 pixels
    xs, w, ref = _size_group(size_refs, c, dtype)
    w = w[:c.cout].contiguous()
    b = rnd((c.cout,), 3, torch.float32, 0.1)
    want = ref[:, :c.cout] + b.double().to(dev()).view(1, -1, 1, 1)
    an = res = None
    if c.epi == "an_relu_res":
        an = (rnd((c.cout,), 5, torch.float32, 0.2), rnd((c.cout,), 6, torch.float32, 0.2))
        want = (want + an[1].double().to(dev()).view(1, -1, 1, 1)) * torch.exp(an[0].double()).to(dev()).view(1, -1, 1, 1)
    if c.epi != "bias":
        res = rnd((B, c.cout, Ho, Wo), 4, dtype)
        want = torch.relu(want) + res.to(dev()).double()
    with ops.tuning({"conv.wlds": c.wlds}):
        got = run_conv(dtype, xs[0], w, b, c.k, c.stride, c.k // 2, an=an, act=0 if c.epi == "bias" else 1, res=res,
                       x2=xs[1] if c.nsrc == 2 else None)
    assert got.shape == want.shape
    d = close_on_device(got, want, tol(dtype, 4 if c.epi == "bias" else 6), c.id)
    print("%s %s: max-abs %.3e" % (c.id, _name(dtype), d))


# ---- b. small non-square geometry, every instantiation a small map reaches at the shipped knobs -------------------------------------------------
# act: 0 none, 1 ReLU, 2 tanh; an: ActNorm folded into the epilogue; nres: residual maps; bar: the tol() scale of the matching test in test_hip_ops.py
GeomCase = collections.namedtuple("GeomCase", "id kind Hin Win cin cout k stride pad reflect nsrc act an nres nchw bar claim")
GEOM_B = 3
GEOM_CASES = (
    GeomCase("k3_s1", "conv", 7, 48, 12, 12, 3, 1, 1, 0, 1, 0, 0, 0, 0, 4, {F16: ("plain", 1, 2), F32: ("plain", 1, 2)}),
    GeomCase("k5_s1", "conv", 7, 48, 3, 24, 5, 1, 2, 0, 1, 1, 0, 0, 0, 4, {F16: ("wl", 2, 1, 4), F32: ("wl", 2, 2, 8)}),
    GeomCase("k3_s2_from_13x95", "conv", 13, 95, 24, 48, 3, 2, 1, 0, 1, 0, 0, 0, 0, 4, {F16: ("wl", 3, 2, 8), F32: ("wl", 3, 2, 8)}),
    GeomCase("reflect7_on_5_rows_tanh_nchw", "conv", 5, 48, 8, 3, 7, 1, 3, 1, 1, 2, 0, 0, 1, 2, {F16: ("plain", 1, 2), F32: ("plain", 1, 2)}),
    GeomCase("k3_nchw_20_channels", "conv", 7, 48, 8, 20, 3, 1, 1, 0, 1, 0, 0, 0, 1, 4, {F16: ("wl", 2, 1, 4), F32: ("wl", 2, 1, 4)}),
    GeomCase("1x1_two_sources", "conv", 7, 48, 48, 48, 1, 1, 0, 0, 2, 1, 1, 2, 0, 6, {F16: ("wl", 3, 1, 4), F32: ("wl", 3, 2, 8)}),
    GeomCase("1x1_three_sources", "conv", 7, 48, 32, 56, 1, 1, 0, 0, 3, 1, 1, 2, 0, 6, {F16: ("wl", 4, 1, 8), F32: ("wl", 4, 1, 8)}),
    GeomCase("k3_88_channels", "conv", 7, 48, 16, 88, 3, 1, 1, 0, 1, 1, 0, 1, 0, 6, {F16: ("wl", 6, 1, 8), F32: ("wl", 6, 1, 8)}),
    GeomCase("k3_120_channels", "conv", 7, 48, 8, 120, 3, 1, 1, 0, 1, 0, 0, 0, 0, 4, {F16: ("plain", 8, 1), F32: ("plain", 8, 1)}),
    # ConvTranspose2d: four phases over the INPUT grid, whose width check_conv wants a multiple of 16
    GeomCase("transposed_5x16", "convT", 5, 16, 24, 12, 4, 2, 1, 0, 1, 1, 0, 0, 0, 4, {F16: ("plain", 1, 2), F32: ("plain", 1, 2)}),
    GeomCase("transposed_5x16_24_channels", "convT", 5, 16, 48, 24, 4, 2, 1, 0, 1, 1, 0, 0, 0, 4, {F16: ("wl", 2, 1, 4), F32: ("wl", 2, 2, 8)}),
)


def geom_out_hw(c):
    if c.kind == "convT":
        return 2 * c.Hin, 2 * c.Win
    return (c.Hin + 2 * c.pad - c.k) // c.stride + 1, (c.Win + 2 * c.pad - c.k) // c.stride + 1


def geom_case_rule(c, dtype):
    Hb, Wb = (c.Hin, c.Win) if c.kind == "convT" else geom_out_hw(c)
    return conv_rules.conv_problem(dtype, GEOM_B, Hb, Wb, c.cin, c.cout, c.k, c.nsrc, transpose=c.kind == "convT")


def G(t, name=None):
    """an input: the operand's values on the device between NaN bands"""
    return guarded_copy(t, device=dev(), name=name)


def O(shape, dtype, name=None):
    """an output on the device, prefilled with 0xff bytes (NaN), between random bands"""
    return guarded_empty(shape, dtype, dev(), "ff", name=name)


def bands(*ts):
    torch.cuda.synchronize()
    check_bands(*[t for t in ts if t is not None])


def padding_zero(out, C, what):
    assert out.shape[-1] > C, "%s: no padding lanes at this shape" % what
    assert float(out[..., C:].float().abs().max()) == 0.0, "%s: padding lanes are not exact zeros" % what


def _affine_ref(y, an, act, res):
    if an:
        y = (y + an[1].double().view(1, -1, 1, 1)) * torch.exp(an[0].double()).view(1, -1, 1, 1)
    y = torch.relu(y) if act == 1 else torch.tanh(y) if act == 2 else y
    for r in res:
        y = y + r.double()
    return y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", GEOM_CASES, ids=[c.id for c in GEOM_CASES])
def test_conv_small_non_square_geometry(c, dtype):
    assert geom_case_rule(c, dtype) == c.claim[_name(dtype)]
    kc, B = conv_rules.kc(dtype), GEOM_B
    Ho, Wo = geom_out_hw(c)
    assert Ho != Wo
    xs = [rnd((B, c.cin, c.Hin, c.Win), 1 + i, dtype) for i in range(c.nsrc)]
    b = rnd((c.cout,), 3, torch.float32, 0.1)
    an = (rnd((c.cout,), 5, torch.float32, 0.2), rnd((c.cout,), 6, torch.float32, 0.2)) if c.an else None
    res = [rnd((B, c.cout, Ho, Wo), 8 + i, dtype) for i in range(c.nres)]
    cin_pad = packing.cs_of(c.cin)
    if c.kind == "convT":
        w = rnd((c.cin, c.cout, 4, 4), 2, dtype, 1 / math.sqrt(c.cin * 4))
        y = F.conv_transpose2d(xs[0].double(), w.double(), b.double(), stride=2, padding=1)
        wp = packing.pack_convT_weight(w, cin_pad, kc, dtype)
    else:
        fan = c.nsrc * c.cin * c.k * c.k
        w = rnd((c.cout, c.nsrc * c.cin, c.k, c.k), 2, dtype, (0.3 if c.act == 2 else 1.0) / math.sqrt(fan))
        xcat = torch.cat(xs, 1).double()
        if c.reflect:
            y = F.conv2d(F.pad(xcat, (c.pad,) * 4, mode="reflect"), w.double(), b.double(), stride=c.stride)
        else:
            y = F.conv2d(xcat, w.double(), b.double(), stride=c.stride, padding=c.pad)
        wp = packing.pack_conv_weight(w, cin_pad, kc, dtype)[0]
    want = _affine_ref(y, an, c.act, res)
    assert tuple(want.shape) == (B, c.cout, Ho, Wo)
    s, t = packing.affine(b, an[0] if an else None, an[1] if an else None, packing.round_up(c.cout, 16))
    gx = [G(ops.to_nhwc(x), "src%d" % i) for i, x in enumerate(xs)]
    gw, gs, gt = G(wp, "w"), G(s, "scale"), G(t, "shift")
    gr = [G(ops.to_nhwc(r), "res%d" % i) for i, r in enumerate(res)]
    out = O((B, c.cout, Ho, Wo), torch.float32, "out NCHW fp32") if c.nchw else O((B, Ho, Wo, packing.round_up(c.cout, 8)), dtype, "out map")
    ops.conv2d(gx[0], gw, gs, gt, cin_pad, c.cout, k=c.k, stride=c.stride, pad=c.pad, reflect=bool(c.reflect), src1=gx[1] if c.nsrc > 1 else None,
               src2=gx[2] if c.nsrc > 2 else None, transpose=c.kind == "convT", act=c.act, res0=gr[0] if c.nres > 0 else None,
               res1=gr[1] if c.nres > 1 else None, nchw_f32=bool(c.nchw), out=out)
    bands(out, gw, gs, gt, *gx, *gr)
    if c.nchw:
        assert out.dtype == torch.float32
        close(out, want, tol(dtype, c.bar), c.id)
    else:
        close(ops.from_nhwc(out, c.cout), want, tol(dtype, c.bar), c.id)
        if out.shape[-1] > c.cout:
            padding_zero(out, c.cout, c.id)
    if c.id == "1x1_two_sources":
        # the residuals are two different maps: a kernel that adds res0 twice, or drops res1, is off by |res1 - res0| or |res1|, far above the bar
        assert float((res[0].double() - res[1].double()).abs().max()) > 1.0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("stride", [1, 2])
def test_conv_one_hot_shift_is_bit_exact_off_square(dtype, stride):
    """out[c](y, x) = in[c + 1](s y - 1, s x + 1), zero outside: every output is a copy of one input (or an exact zero), so a swapped axis, a
    wrong row pitch or a pixel of the neighbouring image shows as a wrong bit.  3 x 7 x 48 outputs; stride 2 from 13 x 95."""
    B, Ho, Wo = GEOM_B, 7, 48
    Hin, Win = (Ho, Wo) if stride == 1 else (13, 95)
    x = rnd((B, 8, Hin, Win), 1, dtype)
    w = torch.zeros(8, 8, 3, 3)
    for ch in range(8):
        w[ch, (ch + 1) % 8, 0, 2] = 1.0
    want = F.conv2d(x.float(), w, stride=stride, padding=1)
    assert tuple(want.shape) == (B, 8, Ho, Wo)
    s, t = packing.affine(torch.zeros(8), cout_pad=16)
    gx, gw, gs, gt = G(ops.to_nhwc(x), "x"), G(packing.pack_conv_weight(w.to(dtype), 8, conv_rules.kc(dtype), dtype)[0], "w"), G(s, "scale"), G(t, "shift")
    out, out32 = O((B, Ho, Wo, 8), dtype, "out map"), O((B, 8, Ho, Wo), torch.float32, "out NCHW fp32")
    ops.conv2d(gx, gw, gs, gt, 8, 8, k=3, stride=stride, pad=1, out=out)
    ops.conv2d(gx, gw, gs, gt, 8, 8, k=3, stride=stride, pad=1, nchw_f32=True, out=out32)
    bands(out, out32, gx, gw, gs, gt)
    assert torch.equal(ops.from_nhwc(out, 8).float().cpu(), want)
    assert torch.equal(out32.cpu(), want)


# ---- c. channel statistics: passes, short and empty chunks, the grid cap ------------------------------------------------------------------------
# expect: what conv_rules.chan_stats_plan / grid_img must say about the shape, per dtype (checked without a GPU and again before the run)
StatsCase = collections.namedtuple("StatsCase", "id C H W dtypes expect")
STATS_B = 2
STATS_CASES = (
    StatsCase("hw40_empty_chunks", 24, 5, 8, (F32, F16), {F32: dict(per=1, empty=24, passes=1, grid=1), F16: dict(per=1, empty=24, passes=1, grid=1)}),
    StatsCase("c128_91x91", 128, 91, 91, (F32, F16),
              {F32: dict(per=130, passes=5, last_pixels=91, empty=0, grid=128), F16: dict(per=130, passes=3, last_pixels=91, empty=0, grid=65)}),
    StatsCase("c128_129x131_grid_cap", 128, 129, 131, (F16,), {F16: dict(per=265, passes=5, last_pixels=204, empty=0, grid=128)}),
    StatsCase("c24_149x151_ragged_lanes", 24, 149, 151, (F32, F16),
              {F32: dict(per=352, lanes=42, idle=4, passes=3, ragged=16, grid=66), F16: dict(per=352, lanes=85, idle=1, passes=2, ragged=12, grid=33)}),
)
STATS_PARAMS = [pytest.param(c, getattr(torch, d), id="%s-%s" % (c.id, d)) for c in STATS_CASES for d in c.dtypes]


def stats_case_facts(c, dtype):
    """conv_rules' account of the case, with the grid of the apply pass"""
    plan = conv_rules.chan_stats_plan(dtype, c.H * c.W, c.C)
    plan["grid"] = conv_rules.grid_img(dtype, c.H * c.W, c.C)
    return plan


def _check_stats_plan(c, dtype):
    facts = stats_case_facts(c, dtype)
    for k, v in c.expect[_name(dtype)].items():
        assert facts[k] == v, "%s %s: %s is %r, the table says %r" % (c.id, _name(dtype), k, facts[k], v)


def _report(what, dtype, r):
    print("%s %s: error / bar %.3g" % (what, _name(dtype), r))
    assert r <= 1.0, "%s %s: error / bar %.3g above 1" % (what, _name(dtype), r)


@pytest.mark.parametrize("c,dtype", STATS_PARAMS)
def test_instnorm_relu_chunking(c, dtype):
    _check_stats_plan(c, dtype)
    x = rnd((STATS_B, c.C, c.H, c.W), 1, dtype, 2.0) + 0.7
    assert not torch.equal(x[0], x[1])
    want = ve.instnorm_relu(x, torch.float64)
    e32 = ve.e32_of(ve.instnorm_relu(x, torch.float32), want)
    xn = G(ops.to_nhwc(x), "map (in place)")
    ops.instnorm_relu_(xn, c.C)
    bands(xn)
    got = ops.from_nhwc(xn, c.C).cpu()
    _report("instnorm_relu %s" % c.id, dtype, ve.ratio(got, want, e32, dtype))
    close(got, want, tol(dtype, 2), c.id)
    close(got, torch.relu(cfen_oracle.instance_norm(x.double())), tol(dtype, 2), c.id + " (oracle)")


@pytest.mark.parametrize("c,dtype", STATS_PARAMS)
def test_cfsm2g_chunking(c, dtype):
    _check_stats_plan(c, dtype)
    C, h = c.C, c.C // 4
    g = torch.Generator().manual_seed(C)
    names = ("fc_avg_cf1", "fc_avg_cf2", "fc_max_cf1", "fc_max_cf2")
    sd = {}
    for fc in names:
        sd["c.%s.0.weight" % fc] = torch.randn(h, C, 1, 1, generator=g) / math.sqrt(C)
        sd["c.%s.2.weight" % fc] = torch.randn(C, h, 1, 1, generator=g) / math.sqrt(h)
    xs = [rnd((STATS_B, C, c.H, c.W), 10 + i, dtype) for i in range(3)]
    assert not torch.equal(xs[0][0], xs[0][1])
    w = torch.cat([sd["c.%s.%d.weight" % (fc, i)].reshape(-1) for fc in names for i in (0, 2)])
    want = cfen_oracle.cfsm2g({k: v.double() for k, v in sd.items()}, "c", *[x.double() for x in xs])
    e32 = ve.e32_of(cfen_oracle.cfsm2g(sd, "c", *[x.float() for x in xs]), want)
    ins = [G(ops.to_nhwc(x), "x%d" % i) for i, x in enumerate(xs)] + [G(w, "gate weights")]
    out = O((STATS_B, c.H, c.W, C), dtype, "out map")
    ops.cfsm2g(*ins, C, out=out)
    bands(out, *ins)
    got = ops.from_nhwc(out, C).cpu()
    _report("cfsm2g %s" % c.id, dtype, ve.ratio(got, want, e32, dtype))
    close(got, want, tol(dtype, 4), c.id)


# ---- d. patchify / unpatchify off square ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify_roundtrip_and_pooled_form_on_32x96(dtype):
    """test_patchify_roundtrip_lvit and test_patchify_pooled_gvit_and_padded_stride (tests/test_hip_ops.py) on H = 32, W = 96: 2 x 6 windows of 16, and
    the pooled 8 x 24 map in three windows of 8; the same bars (exact, exact, tol(dtype))"""
    B, C, H, W, ws = 2, 24, 32, 96, 16
    x = rnd((B, C, H, W), 1, dtype)
    want = perm_tokens(cfen_oracle.unfold_tokens(cfen_oracle.window_partition(x.float(), ws), 2), C, 2).reshape(-1, 4 * C)
    xn = G(ops.to_nhwc(x, cs=32), "fmap")                          # channel stride larger than C
    tok = O(want.shape, dtype, "tokens")
    ops.patchify(xn, C, ws, 2, out=tok)
    bands(xn, tok)
    assert torch.equal(tok.float().cpu(), want)
    gt = G(tok, "tokens in")
    back = O((B, H, W, 32), dtype, "map")
    ops.unpatchify(gt, B, H, W, C, 32, ws, 2, out=back)
    bands(gt, back)
    assert torch.equal(back[..., :C].cpu(), xn[..., :C].cpu())
    pooled = cfen_oracle.avgpool2(cfen_oracle.avgpool2(x.double()))
    want4 = perm_tokens(cfen_oracle.unfold_tokens(cfen_oracle.window_partition(pooled, 8), 4), C, 4).reshape(-1, 16 * C)
    tok4 = O(want4.shape, dtype, "pooled tokens")
    ops.patchify(xn, C, 8, 4, pool=4, out=tok4)
    bands(xn, tok4)
    close(tok4, want4, tol(dtype))
