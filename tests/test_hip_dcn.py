"""GPU parity of the HIP deformable-conv operator (through the reference-shaped Python API and the C ABI)
against the C oracle, on the feature-map shapes of the v3 generator and the edge cases
the reference's Python layer guards; from "geometry that tells h from w" on also against tests/dcn_ref.py
(float64, gradients by autograd), the pin of the oracle itself (tests/test_dcn_oracle.py)."""
import pytest
import torch
import torch.nn.functional as F

import dcn_oracle
import dcn_ref
from cfen_vit_dehazing_amd import _lib, dcn, ops
from cfen_vit_dehazing_amd._lib import check, current_stream, dtype_code, ptr
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def tol(dtype):
    return 2e-4 if dtype == torch.float32 else 2e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,C,H,Cout,k,stride,pad,dil,groups,dg", [
    (2, 24, 32, 24, 3, 1, 1, 1, 1, 1), (1, 48, 16, 48, 3, 1, 1, 1, 1, 8), (1, 96, 16, 96, 3, 1, 1, 1, 1, 8),
    (2, 8, 13, 6, 3, 2, 1, 1, 1, 2), (1, 8, 12, 12, 5, 1, 2, 1, 2, 1), (1, 6, 10, 160, 3, 1, 2, 2, 1, 3), (3, 3, 9, 5, 1, 1, 0, 1, 1, 1),
    # k_dcn_lean: two conv groups of 24 channels cut into deformable groups of 12, stride / dilation 2 with 40 output rows and groups of 3,
    # two output-row blocks, a 5x5 kernel (three tap slices, the last one padded), a unit inside a 48-channel deformable group
    (1, 48, 16, 48, 3, 1, 1, 1, 2, 4), (2, 24, 17, 40, 3, 2, 2, 2, 1, 8), (1, 24, 12, 160, 3, 1, 1, 1, 1, 1), (1, 24, 14, 24, 5, 1, 2, 1, 1, 4),
    (1, 96, 12, 48, 3, 1, 1, 1, 1, 2)])
def test_deform_conv_v1_and_v2(dtype, B, C, H, Cout, k, stride, pad, dil, groups, dg):
    x, w = rnd((B, C, H, H + 3), 1), rnd((Cout, C // groups, k, k), 2, (C // groups * k * k) ** -0.5)
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    Wo = (H + 3 + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    off = rnd((B, dg * 2 * k * k, Ho, Wo), 3, 2.0)
    mask = torch.sigmoid(rnd((B, dg * k * k, Ho, Wo), 4))
    bias = rnd((Cout,), 5)
    xq, wq, oq, mq, bq = (t.to(dtype) for t in (x, w, off, mask, bias))
    want1 = dcn_oracle.deform_conv(xq.float(), oq.float(), wq.float(), stride, pad, dil, groups, dg)
    got1 = dcn.deform_conv(xq.to(DEV), oq.to(DEV), wq.to(DEV), stride, pad, dil, groups, dg)
    assert got1.dtype == dtype and got1.shape == want1.shape
    assert float((got1.float().cpu() - want1).abs().max()) <= tol(dtype)
    want2 = dcn_oracle.deform_conv(xq.float(), oq.float(), wq.float(), stride, pad, dil, groups, dg, mask=mq.float(), bias=bq.float())
    got2 = dcn.modulated_deform_conv(xq.to(DEV), oq.to(DEV), mq.to(DEV), wq.to(DEV), bq.to(DEV), stride, pad, dil, groups, dg)
    assert float((got2.float().cpu() - want2).abs().max()) <= tol(dtype)


@pytest.mark.parametrize("C,dg", [(24, 1), (24, 8), (48, 8), (96, 8)])
def test_lean_kernel_and_round2_kernel_agree(C, dg):
    """`dcn.tile` 0 runs k_dcn_nhwc (round 2) on the shapes k_dcn_lean serves by default: same sampling rules; the lean kernel interpolates
    fp16 maps with packed fp16 FMAs (as the reference's half instantiation does), k_dcn_nhwc in fp32 -- equal to fp16 rounding of the samples."""
    from cfen_vit_dehazing_amd import ops
    H = 40
    x, w = rnd((2, C, H, H), 21).half().to(DEV), rnd((C, C, 3, 3), 22, (C * 9) ** -0.5).half().to(DEV)
    off = rnd((2, dg * 18, H, H), 23, 3.0).half().to(DEV)
    mask = torch.sigmoid(rnd((2, dg * 9, H, H), 24)).half().to(DEV)
    bias = rnd((C,), 25).half().to(DEV)
    got = []
    for t in (1, 0):
        with ops.tuning({"dcn.tile": t}):
            got.append((dcn.deform_conv(x, off, w, 1, 1, 1, 1, dg), dcn.modulated_deform_conv(x, off, mask, w, bias, 1, 1, 1, 1, dg)))
    for a, b in zip(got[0], got[1]):
        assert float((a.float() - b.float()).abs().max()) <= 8e-3


@pytest.mark.parametrize("dtype,C,dg", [(torch.float16, 24, 1), (torch.float16, 48, 8), (torch.float32, 24, 4)])
def test_channels_last_input_skips_the_layout_pass_and_gives_the_same_bits(dtype, C, dg):
    """(extension, round 6) an undifferentiated call on a channels_last input samples from the tensor's own NHWC memory (cfen_*_forward_nhwc): bit for bit the result of
    the contiguous call, v1 and v2; a differentiated call keeps the NCHW copy (its backward kernels read NCHW)"""
    d = "cuda:0"
    g = torch.Generator().manual_seed(7)
    B, H = 2, 40
    x = torch.randn(B, C, H, H, generator=g).to(dtype).to(d)
    w = (torch.randn(C, C, 3, 3, generator=g) * (C * 9) ** -0.5).to(dtype).to(d)
    off = (torch.randn(B, dg * 18, H, H, generator=g) * 2.0).to(dtype).to(d)
    mask = torch.sigmoid(torch.randn(B, dg * 9, H, H, generator=g)).to(dtype).to(d)
    bias = torch.randn(C, generator=g).to(dtype).to(d)
    xcl = x.contiguous(memory_format=torch.channels_last)
    assert not xcl.is_contiguous()
    with torch.no_grad():
        assert torch.equal(dcn.deform_conv(xcl, off, w, 1, 1, 1, 1, dg), dcn.deform_conv(x, off, w, 1, 1, 1, 1, dg))
        assert torch.equal(dcn.modulated_deform_conv(xcl, off, mask, w, bias, 1, 1, 1, 1, dg), dcn.modulated_deform_conv(x, off, mask, w, bias, 1, 1, 1, 1, dg))
    xg = xcl.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    y = dcn.deform_conv(xg, off, w, 1, 1, 1, 1, dg)
    y.float().sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()


def test_pack_modules_at_init_are_plain_convs():
    # DeformConvPack zero-initialises conv_offset (deform_conv.py:211-213) => plain conv
    torch.manual_seed(0)
    m = dcn.DeformConvPack(24, 24, 3, stride=1, padding=1, deformable_groups=8).to(DEV)
    x = rnd((2, 24, 32, 32), 1).to(DEV)
    want = F.conv2d(x.cpu(), m.weight.detach().cpu(), padding=1)
    assert float((m(x).cpu() - want).abs().max()) <= 2e-4
    m2 = dcn.ModulatedDeformConvPack(24, 12, 3, stride=1, padding=1, deformable_groups=2, bias=True).to(DEV)
    with torch.no_grad():
        m2.bias.copy_(rnd((12,), 2))
    want2 = 0.5 * F.conv2d(x.cpu(), m2.weight.detach().cpu(), padding=1) + m2.bias.detach().cpu().view(1, -1, 1, 1)   # sigmoid(0) = 0.5
    assert float((m2(x).cpu() - want2).abs().max()) <= 2e-4
    m3 = dcn.ModulatedDeformConvPack2(24, 12, 3, stride=1, padding=1, extra_offset_mask=True, offset_in_channel=8).to(DEV)
    feat = rnd((2, 8, 32, 32), 3).to(DEV)
    assert m3([x, feat]).shape == (2, 12, 32, 32)


def test_error_behaviour_matches_reference():
    x = torch.zeros(2, 4, 8, 8, device=DEV)
    w = torch.zeros(4, 4, 3, 3, device=DEV)
    with pytest.raises(ValueError):
        dcn.deform_conv(torch.zeros(4, 8, 8, device=DEV), torch.zeros(1, device=DEV), w)            # not 4-D (deform_conv.py:19-21)
    with pytest.raises(ValueError):
        dcn.deform_conv(torch.zeros(1, 4, 2, 2, device=DEV), torch.zeros(1, 18, 1, 1, device=DEV), w)  # output too small (:91-93)
    with pytest.raises(AssertionError):
        dcn.deform_conv(torch.zeros(3, 4, 8, 8, device=DEV), torch.zeros(3, 18, 8, 8, device=DEV), w, 1, 1, 1, 1, 1, 2)  # step !| batch (:40)
    with pytest.raises(NotImplementedError):
        dcn.deform_conv(x.cpu(), torch.zeros(2, 18, 8, 8), w.cpu(), 1, 1)                           # CPU tensors (:36-37)
    with pytest.raises(RuntimeError):
        dcn.deform_conv(x, torch.zeros(2, 16, 8, 8, device=DEV), w, 1, 1)                            # offset channels (.cpp:129-130)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C,H,dg", [(24, 256, 1), (24, 256, 8), (48, 128, 1), (48, 128, 8), (96, 64, 1), (96, 64, 8)])
def test_deform_conv_at_the_generator_feature_map_shapes(dtype, C, H, dg):
    """(B,24,256,256) / (B,48,128,128) / (B,96,64,64), 3x3 s1 p1, deformable groups 1 and 8, v1 and v2.
    Batch 2 (the oracle is scalar C); offsets of +-2 pixels reach over the borders."""
    B = 2
    x, w = rnd((B, C, H, H), 11), rnd((C, C, 3, 3), 12, (C * 9) ** -0.5)
    off = rnd((B, dg * 18, H, H), 13, 2.0)
    mask = torch.sigmoid(rnd((B, dg * 9, H, H), 14))
    bias = rnd((C,), 15)
    xq, wq, oq, mq, bq = (t.to(dtype) for t in (x, w, off, mask, bias))
    want1 = dcn_oracle.deform_conv(xq.float(), oq.float(), wq.float(), 1, 1, 1, 1, dg)
    got1 = dcn.deform_conv(xq.to(DEV), oq.to(DEV), wq.to(DEV), 1, 1, 1, 1, dg)
    assert float((got1.float().cpu() - want1).abs().max()) <= tol(dtype)
    want2 = dcn_oracle.deform_conv(xq.float(), oq.float(), wq.float(), 1, 1, 1, 1, dg, mask=mq.float(), bias=bq.float())
    got2 = dcn.modulated_deform_conv(xq.to(DEV), oq.to(DEV), mq.to(DEV), wq.to(DEV), bq.to(DEV), 1, 1, 1, 1, dg)
    assert float((got2.float().cpu() - want2).abs().max()) <= tol(dtype)


# ---- backward (csrc/k_dcn_bwd.hip) through autograd of the reference-shaped functions, against oracle/dcn_oracle.c -----------------------

def _grad_close(got, want, dtype, what):
    scale = max(1.0, float(want.abs().max()))
    d = float((got.float().cpu() - want).abs().max())
    bar = (3e-4 if dtype == torch.float32 else 2e-2) * scale
    assert d <= bar, "%s: max-abs %.3e > %.1e (scale %.2f)" % (what, d, bar, scale)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,C,H,Cout,k,stride,pad,dil,groups,dg", [
    (2, 24, 16, 24, 3, 1, 1, 1, 1, 1), (1, 48, 12, 48, 3, 1, 1, 1, 1, 8), (2, 8, 13, 6, 3, 2, 1, 1, 1, 2), (1, 8, 12, 12, 5, 1, 2, 1, 2, 1),
    (1, 6, 10, 20, 3, 1, 2, 2, 1, 3), (3, 3, 9, 5, 1, 1, 0, 1, 1, 1)])
def test_deform_conv_backward_v1_and_v2(dtype, B, C, H, Cout, k, stride, pad, dil, groups, dg):
    x, w = rnd((B, C, H, H + 3), 1), rnd((Cout, C // groups, k, k), 2, (C // groups * k * k) ** -0.5)
    Ho = (H + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    Wo = (H + 3 + 2 * pad - (dil * (k - 1) + 1)) // stride + 1
    off, mask, bias = rnd((B, dg * 2 * k * k, Ho, Wo), 3, 1.5), torch.rand(B, dg * k * k, Ho, Wo, generator=torch.Generator().manual_seed(4)), rnd((Cout,), 5)
    gy = rnd((B, Cout, Ho, Wo), 6)
    if dtype == torch.float16:                  # the oracle sees what the kernel sees
        x, w, off, mask, gy = (t.half().float() for t in (x, w, off, mask, gy))
    leaf = lambda t: t.to(DEV).to(dtype).requires_grad_()
    # DCNv1
    xi, oi, wi = leaf(x), leaf(off), leaf(w)
    y = dcn.deform_conv(xi, oi, wi, stride, pad, dil, groups, dg)
    y.backward(gy.to(DEV).to(dtype))
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, stride, pad, dil, groups, dg)
    _grad_close(xi.grad, want["input"], dtype, "v1 grad_input")
    _grad_close(oi.grad, want["offset"], dtype, "v1 grad_offset")
    _grad_close(wi.grad, want["weight"], dtype, "v1 grad_weight")
    # DCNv2 (+ mask, + bias)
    xi, oi, mi, wi, bi = leaf(x), leaf(off), leaf(mask), leaf(w), leaf(bias)
    y = dcn.modulated_deform_conv(xi, oi, mi, wi, bi, stride, pad, dil, groups, dg)
    y.backward(gy.to(DEV).to(dtype))
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, stride, pad, dil, groups, dg, mask=mask, with_bias=True)
    for name, t in (("input", xi), ("offset", oi), ("mask", mi), ("weight", wi), ("bias", bi)):
        _grad_close(t.grad, want[name], dtype, "v2 grad_" + name)


def test_deform_conv_backward_only_weight_or_only_input_is_requested():
    """dcn/deform_conv.py:62-80: the two extension calls are made independently, by needs_input_grad"""
    x, w, off = rnd((1, 8, 10, 10), 1), rnd((8, 8, 3, 3), 2, 0.2), rnd((1, 18, 10, 10), 3)
    gy = rnd((1, 8, 10, 10), 4)
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, 1, 1)
    wi = w.to(DEV).requires_grad_()
    dcn.deform_conv(x.to(DEV), off.to(DEV), wi, 1, 1, 1, 1, 1).backward(gy.to(DEV))
    _grad_close(wi.grad, want["weight"], torch.float32, "grad_weight alone")
    xi = x.to(DEV).requires_grad_()
    dcn.deform_conv(xi, off.to(DEV), w.to(DEV), 1, 1, 1, 1, 1).backward(gy.to(DEV))
    _grad_close(xi.grad, want["input"], torch.float32, "grad_input alone")


def test_deform_conv_pack_trains_one_sgd_step_like_conv2d_at_init():
    """DeformConvPack at init (zero offset conv) is a plain conv: its weight gradient equals conv2d's (deform_conv.py:222-231)"""
    torch.manual_seed(0)
    m = dcn.DeformConvPack(8, 8, 3, stride=1, padding=1, deformable_groups=2).to(DEV)
    x = rnd((2, 8, 12, 12), 7).to(DEV)
    y = m(x)
    y.square().mean().backward()
    w = m.weight.detach().clone().requires_grad_()
    F.conv2d(x, w, None, 1, 1).square().mean().backward()
    assert float((m.weight.grad - w.grad).abs().max()) <= 2e-5


@pytest.mark.parametrize("off_scale", [1.0, 12.0])
def test_deform_conv_backward_lds_col2im_equals_global_atomics(off_scale):
    """grad_input through the LDS-privatised col2im with parked tiles (1, default), with tiles flushed by global atomics (2) and through
    plain global atomics (0); small offsets (all inside the tile halo) and offsets far beyond it (the per-add fallback to global memory),
    40 x 36 pixels so that tiles are ragged; all against the oracle"""
    from cfen_vit_dehazing_amd import _lib
    x, w = rnd((2, 12, 40, 36), 1), rnd((12, 12, 3, 3), 2, 0.15)
    off, gy = rnd((2, 36, 40, 36), 3, off_scale), rnd((2, 12, 40, 36), 4)
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, 1, 2)
    lib = _lib.load()
    got = {}
    for lds in (1, 2, 0):
        old = lib.cfen_deform_conv_backward_set_lds(lds)
        try:
            xi = x.to(DEV).requires_grad_()
            dcn.deform_conv(xi, off.to(DEV), w.to(DEV), 1, 1, 1, 1, 2).backward(gy.to(DEV))
            got[lds] = xi.grad.cpu()
        finally:
            lib.cfen_deform_conv_backward_set_lds(old)
        _grad_close(got[lds], want["input"], torch.float32, "grad_input (lds=%d)" % lds)
    for lds in (1, 2):
        assert float((got[lds] - got[0]).abs().max()) <= 1e-4 * max(1.0, float(want["input"].abs().max()))


def test_deform_conv_backward_fixed_point_col2im_edge_cases():
    """k_dcnb_col2im_lds accumulates in 64-bit fixed point scaled by the workgroup's largest contribution: the result must not depend on
    the magnitude of the gradients (power-of-two scalings are exact, so grad_input scales BITWISE), an all-zero grad_output gives exact zeros,
    run-to-run results are bit-identical (the adds are order-independent; offsets stay inside the tile halo so no global atomics are
    involved), and a non-finite grad_output is not laundered into finite numbers."""
    x, w = rnd((2, 16, 24, 20), 1), rnd((8, 16, 3, 3), 2, 0.1)
    off, gy = rnd((2, 18, 24, 20), 3, 1.0), rnd((2, 8, 24, 20), 4)

    def grad_in(g):
        xi = x.to(DEV).requires_grad_()
        dcn.deform_conv(xi, off.to(DEV), w.to(DEV), 1, 1, 1, 1, 1).backward(g.to(DEV))
        return xi.grad.cpu()

    base = grad_in(gy)
    _grad_close(base, dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, 1, 1)["input"], torch.float32, "grad_input")
    assert torch.equal(grad_in(gy), base)                                        # deterministic
    for k in (-60, -20, 20, 60):
        assert torch.equal(grad_in(gy * 2.0 ** k), base * 2.0 ** k), "scale 2^%d" % k
    assert torch.equal(grad_in(torch.zeros_like(gy)), torch.zeros_like(base))
    for poison in (float("inf"), float("nan")):
        bad = gy.clone()
        bad[1, 3, 10, 7] = poison
        g = grad_in(bad)
        assert not bool(torch.isfinite(g[1]).all()) and bool(torch.isfinite(g[0]).all())


# ---- geometry that tells h from w ----------------------------------------------------------------------------------------------------------
# The v1 entry points take (kW, kH, dW, dH, padW, padH, dilationW, dilationH), the v2 entry points h before w, and dcn/deform_conv.py swaps the
# pairs by hand; everything above passes square kernels and scalar stride / padding / dilation, which no swap can change.  From here on every
# h / w pair differs somewhere, the expected values come from the oracle AND (the cases are small) from tests/dcn_ref.py, and the bars are
# the ones above: tol(dtype) for outputs, _grad_close for gradients.

def _problem(B, C, H, W, Cout, k, s, p, d, groups, dg, dtype, seed=50, off_scale=2.0):
    """float32 CPU tensors holding values of `dtype` (the oracle sees what the kernel sees)"""
    Ho, Wo = dcn_ref.out_size(H, W, k, s, p, d)
    kk, Cg = k[0] * k[1], C // groups
    q = lambda t: t.to(dtype).float()
    x, w = q(rnd((B, C, H, W), seed + 1)), q(rnd((Cout, Cg, k[0], k[1]), seed + 2, (Cg * kk) ** -0.5))
    off = q(dcn_ref.keep_off_integers(rnd((B, dg * 2 * kk, Ho, Wo), seed + 3, off_scale)))
    mask = q(torch.rand(B, dg * kk, Ho, Wo, generator=torch.Generator().manual_seed(seed + 4)))
    return x, w, off, mask, q(rnd((Cout,), seed + 5)), q(rnd((B, Cout, Ho, Wo), seed + 6))


def _v2_forward_c(x, off, mask, w, bias, s, p, d, groups, dg):
    """cfen_modulated_deform_conv_forward by ctypes (h before w); scratch as dcn/deform_conv.py's _columns allocates it"""
    lib, dt = _lib.load(), dtype_code(x.dtype)
    B, C, H, W = x.shape
    Cout, _, kh, kw = w.shape
    Ho, Wo = dcn_ref.out_size(H, W, (kh, kw), s, p, d)
    out = x.new_empty(B, Cout, Ho, Wo)
    n = int(lib.cfen_deform_conv_columns_bytes(dt, B, C, H, W, Cout, kh, kw, groups))
    columns = torch.empty(max(n, 16), dtype=torch.uint8, device=x.device)
    check(lib.cfen_modulated_deform_conv_forward(dt, ptr(x), ptr(w), ptr(bias), ptr(off), ptr(mask), ptr(out), B, C, H, W, Cout, kh, kw, s[0], s[1],
                                                 p[0], p[1], d[0], d[1], groups, dg, int(bias is not None), ptr(columns), n, current_stream()),
          "modulated_deform_conv_forward")
    return out


def _v2_backward_c(x, off, mask, w, gy, s, p, d, groups, dg):
    """cfen_modulated_deform_conv_backward by ctypes; zeroed gradients and scratch as ModulatedDeformConvFunction.backward / _backward_scratch make them"""
    lib, dt = _lib.load(), dtype_code(x.dtype)
    B, C, H, W = x.shape
    Cout, _, kh, kw = w.shape
    g = {"input": torch.zeros_like(x), "offset": torch.zeros_like(off), "mask": torch.zeros_like(mask), "weight": torch.zeros_like(w),
         "bias": torch.zeros(Cout, dtype=x.dtype, device=x.device)}
    n = int(lib.cfen_deform_conv_backward_bytes(B, C, H, W, Cout, kh, kw, gy.shape[2], gy.shape[3], groups))
    columns = torch.empty(max(n, 16), dtype=torch.uint8, device=x.device)
    check(lib.cfen_modulated_deform_conv_backward(dt, ptr(x), ptr(w), None, ptr(off), ptr(mask), ptr(g["input"]), ptr(g["weight"]), ptr(g["bias"]),
                                                  ptr(g["offset"]), ptr(g["mask"]), ptr(gy), B, C, H, W, Cout, kh, kw, s[0], s[1], p[0], p[1], d[0], d[1],
                                                  groups, dg, 1, ptr(columns), n, current_stream()), "modulated_deform_conv_backward")
    return g


def _ref_backward(x, off, w, gy, s, p, d, groups, dg, mask=None, bias=None):
    """tests/dcn_ref.py: gradients of <output, gy> by autograd, float64"""
    leaves = {"input": x, "offset": off, "weight": w}
    if mask is not None:
        leaves.update(mask=mask, bias=bias)
    leaves = {n: t.double().requires_grad_() for n, t in leaves.items()}
    dcn_ref.deform_conv_f64(leaves["input"], leaves["offset"], leaves["weight"], s, p, d, groups, dg, mask=leaves.get("mask"),
                            bias=leaves.get("bias")).backward(gy.double())
    return {n: t.grad for n, t in leaves.items()}


def _out_close(got, wants, dtype, what):
    for ref, want in wants.items():
        assert got.shape == want.shape, what
        dist = float((got.float().cpu().double() - want.double()).abs().max())
        print("%s vs %s: %.3e" % (what, ref, dist))
        assert dist <= tol(dtype), "%s vs %s: max-abs %.3e > %.1e" % (what, ref, dist, tol(dtype))


# (B, C, H, W, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), groups, deformable groups)
HW_GEOMETRIES = {
    "1x3_s12_p01_d12_g2_dg2": (2, 8, 13, 17, 6, (1, 3), (1, 2), (0, 1), (1, 2), 2, 2),
    "3x1_s21_p10_d21_g1_dg8": (2, 24, 14, 11, 24, (3, 1), (2, 1), (1, 0), (2, 1), 1, 8),
    "3x2_s12_p21_g2_dg4_cout80": (1, 48, 12, 15, 80, (3, 2), (1, 2), (2, 1), (1, 1), 2, 4),
    "5x3_s21_p23_d12_g2_dg6": (2, 12, 11, 9, 6, (5, 3), (2, 1), (2, 3), (1, 2), 2, 6),
    "2x4_s13_p12_d31_g1_dg2": (3, 16, 9, 16, 8, (2, 4), (1, 3), (1, 2), (3, 1), 1, 2),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("name", list(HW_GEOMETRIES))
def test_forward_on_geometry_that_tells_h_from_w(name, dtype):
    """v1 through dcn.deform_conv with tuple stride / padding / dilation; v2 with distinct pairs through cfen_modulated_deform_conv_forward, and with
    the non-square kernel through dcn.modulated_deform_conv (scalar stride / padding / dilation, the reference's signature)"""
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    x, w, off, mask, bias, _ = _problem(*HW_GEOMETRIES[name], dtype)
    dev = lambda t: t.to(DEV).to(dtype)
    got = dcn.deform_conv(dev(x), dev(off), dev(w), s, p, d, groups, dg)
    assert got.dtype == dtype
    _out_close(got, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg), "float64": dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg)},
               dtype, "v1")
    got = _v2_forward_c(dev(x), dev(off), dev(mask), dev(w), dev(bias), s, p, d, groups, dg)
    _out_close(got, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias),
                     "float64": dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)}, dtype, "v2 (C ABI)")
    s1, p1, d1 = s[0], p[0], d[0]                            # the Python function's scalars; the kernel stays non-square
    x, w, off, mask, bias, _ = _problem(B, C, H, W, Cout, k, (s1, s1), (p1, p1), (d1, d1), groups, dg, dtype, seed=60)
    got = dcn.modulated_deform_conv(dev(x), dev(off), dev(mask), dev(w), dev(bias), s1, p1, d1, groups, dg)
    _out_close(got, {"oracle": dcn_oracle.deform_conv(x, off, w, s1, p1, d1, groups, dg, mask=mask, bias=bias),
                     "float64": dcn_ref.deform_conv_f64(x, off, w, s1, p1, d1, groups, dg, mask=mask, bias=bias)}, dtype, "v2 (Python)")


def _grads_close(got, wants, dtype, what):
    for ref, want in wants.items():
        for name, g in got.items():
            _grad_close(g, want[name].float(), dtype, "%s grad_%s vs %s" % (what, name, ref))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("name", list(HW_GEOMETRIES))
def test_backward_on_geometry_that_tells_h_from_w(name, dtype):
    """all gradients: v1 by autograd of dcn.deform_conv (cfen_deform_conv_backward_input / _parameters, W before H), v2 through
    cfen_modulated_deform_conv_backward with distinct pairs and by autograd of dcn.modulated_deform_conv with the non-square kernel"""
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    x, w, off, mask, bias, gy = _problem(*HW_GEOMETRIES[name], dtype, off_scale=1.5)
    dev = lambda t: t.to(DEV).to(dtype)
    leaf = lambda t: dev(t).requires_grad_()
    xi, oi, wi = leaf(x), leaf(off), leaf(w)
    dcn.deform_conv(xi, oi, wi, s, p, d, groups, dg).backward(dev(gy))
    _grads_close({"input": xi.grad, "offset": oi.grad, "weight": wi.grad},
                 {"oracle": dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg), "float64": _ref_backward(x, off, w, gy, s, p, d, groups, dg)},
                 dtype, "v1")
    got = _v2_backward_c(dev(x), dev(off), dev(mask), dev(w), dev(gy), s, p, d, groups, dg)
    _grads_close(got, {"oracle": dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg, mask=mask, with_bias=True),
                       "float64": _ref_backward(x, off, w, gy, s, p, d, groups, dg, mask=mask, bias=bias)}, dtype, "v2 (C ABI)")
    s1, p1, d1 = s[0], p[0], d[0]
    x, w, off, mask, bias, gy = _problem(B, C, H, W, Cout, k, (s1, s1), (p1, p1), (d1, d1), groups, dg, dtype, seed=60, off_scale=1.5)
    xi, oi, mi, wi, bi = leaf(x), leaf(off), leaf(mask), leaf(w), leaf(bias)
    dcn.modulated_deform_conv(xi, oi, mi, wi, bi, s1, p1, d1, groups, dg).backward(dev(gy))
    _grads_close({"input": xi.grad, "offset": oi.grad, "mask": mi.grad, "weight": wi.grad, "bias": bi.grad},
                 {"oracle": dcn_oracle.deform_conv_backward(x, off, w, gy, s1, p1, d1, groups, dg, mask=mask, with_bias=True),
                  "float64": _ref_backward(x, off, w, gy, (s1, s1), (p1, p1), (d1, d1), groups, dg, mask=mask, bias=bias)}, dtype, "v2 (Python)")


# ---- every forward kernel instance ------------------------------------------------------------------------------------------------------

def _forward_kernel(dtype, C, groups, dg, Cout, knobs):
    """launch_dcn's and dcn_lean_mode's rules (csrc/k_dcn.hip), restated: VE = channels per 16 bytes, UNIT = 3 VE.
      k_dcn        C / groups is not a multiple of VE (dcn_use_scratch leaves the NHWC copy out)
      k_dcn_nhwc   `dcn.tile` 0, or C / groups is not a multiple of UNIT, or C / dg fits none of the lean modes
      lean1        C / dg is a multiple of UNIT (a unit lies inside one deformable group)
      lean3/6/12   C / dg is 3, 6 (or, fp16 only, 12): a unit walks through UNIT / (C / dg) deformable groups
    and the lean kernel keeps 3 accumulators per wave for up to 32 output channels per group (rounded up to 16), 11 beyond."""
    ve = 4 if dtype == torch.float32 else 8
    unit, Cg, cpdg = 3 * ve, C // groups, C // dg
    if Cg % ve:
        return "k_dcn"
    if knobs.get("dcn.tile", 1) == 0 or Cg % unit:
        return "k_dcn_nhwc"
    if cpdg % unit == 0:
        mode = 1
    elif unit % cpdg == 0 and (cpdg in (3, 6) or (cpdg == 12 and ve == 8)):
        mode = cpdg
    else:
        return "k_dcn_nhwc"
    return "lean%d_acc%d" % (mode, 3 if (min(128, Cout // groups) + 15) // 16 * 16 <= 32 else 11)


F32, F16 = torch.float32, torch.float16
# id = <kernel instance>-<dtype>-<what selects it>: (dtype, C, groups, dg, Cout, knobs); each runs without (v1) and with (v2) a mask
FORWARD_INSTANCES = {
    "k_dcn-fp32-6_channels_per_group": (F32, 12, 2, 3, 10, {}),
    "k_dcn-fp16-12_channels_per_group": (F16, 12, 1, 3, 10, {}),
    "k_dcn_nhwc-fp32-tile_0": (F32, 24, 1, 2, 24, {"dcn.tile": 0}),                  # C / dg a multiple of VE: the two-vector fast path
    "k_dcn_nhwc-fp16-tile_0": (F16, 24, 1, 1, 24, {"dcn.tile": 0}),
    "k_dcn_nhwc-fp32-8_channels_per_group": (F32, 16, 2, 8, 12, {}),                 # 8 % 12 != 0; C / dg = 2: a vector straddles deformable groups
    "k_dcn_nhwc-fp16-16_channels_per_group": (F16, 32, 2, 8, 12, {}),                # 16 % 24 != 0; C / dg = 4
    "lean1_acc3-fp32-12_per_dg": (F32, 24, 1, 2, 24, {}),
    "lean1_acc11-fp32-12_per_dg_2_groups": (F32, 24, 2, 2, 80, {}),
    "lean1_acc3-fp16-24_per_dg_2_groups": (F16, 48, 2, 2, 48, {}),
    "lean1_acc11-fp16-24_per_dg": (F16, 24, 1, 1, 40, {}),
    "lean3_acc3-fp32": (F32, 24, 1, 8, 24, {}),
    "lean3_acc11-fp32": (F32, 24, 1, 8, 48, {}),
    "lean3_acc3-fp16": (F16, 24, 1, 8, 24, {}),
    "lean3_acc11-fp16": (F16, 24, 1, 8, 48, {}),
    "lean6_acc3-fp32": (F32, 24, 1, 4, 24, {}),
    "lean6_acc11-fp32": (F32, 24, 2, 4, 96, {}),
    "lean6_acc3-fp16": (F16, 24, 1, 4, 32, {}),
    "lean6_acc11-fp16": (F16, 48, 2, 8, 96, {}),
    "lean12_acc3-fp16": (F16, 24, 1, 2, 24, {}),
    "lean12_acc11-fp16": (F16, 48, 2, 4, 80, {}),
    # six taps in slices of 4 + 2 and of one tap each (`dcn.tps` caps the taps per slice; by default all six fit one slice)
    "lean1_acc3-fp32-tps_4": (F32, 24, 1, 2, 24, {"dcn.tps": 4}),
    "lean3_acc3-fp16-tps_1": (F16, 24, 1, 8, 24, {"dcn.tps": 1}),
    "lean6_acc11-fp32-tps_1": (F32, 24, 1, 4, 48, {"dcn.tps": 1}),
    "lean12_acc3-fp16-tps_4": (F16, 24, 1, 2, 24, {"dcn.tps": 4}),
}


@pytest.mark.parametrize("name", list(FORWARD_INSTANCES))
def test_every_forward_kernel_instance_on_geometry_that_tells_h_from_w(name):
    """3 x 2 kernel, stride (1, 2), padding (2, 1), dilation (2, 1) on 13 x 18 pixels: 130 output pixels, the third workgroup ragged"""
    dtype, C, groups, dg, Cout, knobs = FORWARD_INSTANCES[name]
    assert name.startswith(_forward_kernel(dtype, C, groups, dg, Cout, knobs) + "-"), "the case no longer selects the kernel it is named after"
    k, s, p, d = (3, 2), (1, 2), (2, 1), (2, 1)
    x, w, off, mask, bias, _ = _problem(2, C, 13, 18, Cout, k, s, p, d, groups, dg, dtype, seed=70)
    dev = lambda t: t.to(DEV).to(dtype)
    with ops.tuning(knobs):
        got1 = dcn.deform_conv(dev(x), dev(off), dev(w), s, p, d, groups, dg)
        got2 = _v2_forward_c(dev(x), dev(off), dev(mask), dev(w), dev(bias), s, p, d, groups, dg)
    _out_close(got1, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg), "float64": dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg)},
               dtype, "v1")
    _out_close(got2, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias),
                      "float64": dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)}, dtype, "v2")


# ---- samples on the operator's edges ----------------------------------------------------------------------------------------------------
# Each kernel's bounds test was read before these ran: k_dcn and k_dcn_nhwc compare the float position against (-1, H) / (-1, W) and only then (k_dcn,
# k_dcn_nhwc's general path) convert it, or (k_dcn_nhwc's two-vector path) convert first, to an int that +-70 000 fits, and clamp the corner
# indices before they address anything; k_dcn_lean's dcn_axis takes both per-axis weights from float comparisons and clamps floor(c) into [0, n - 1]
# BEFORE the 24-bit multiplies, so those only ever see a row or column index of the image.

EDGE_INSTANCES = {
    "k_dcn-fp32": (F32, 6, 1, 2, 10, {}), "k_dcn-fp16": (F16, 12, 1, 3, 10, {}),
    "k_dcn_nhwc-fp32-tile_0": (F32, 24, 1, 2, 24, {"dcn.tile": 0}), "k_dcn_nhwc-fp16-tile_0": (F16, 24, 1, 1, 24, {"dcn.tile": 0}),
    "k_dcn_nhwc-fp32-straddling_vectors": (F32, 8, 1, 4, 12, {}),
    "lean1_acc3-fp32": (F32, 24, 1, 1, 24, {}), "lean1_acc3-fp16": (F16, 24, 1, 1, 24, {}),
    "lean3_acc3-fp32": (F32, 24, 1, 8, 24, {}), "lean3_acc3-fp16": (F16, 24, 1, 8, 24, {}),
    "lean6_acc11-fp32": (F32, 24, 1, 4, 48, {}), "lean12_acc3-fp16": (F16, 24, 1, 2, 24, {}),
}


@pytest.mark.parametrize("name", list(EDGE_INSTANCES))
def test_samples_on_the_edges_and_far_off_the_image(name):
    """samples exactly at -1, -0.5, 0, n - 1, n - 0.5, n per axis (every pair of row and column position), at integers, and 70 000 (fp32) or about
    60 000 (fp16: the largest offsets the type holds) pixels off the image: legal inputs, zero beyond the (-1, n) bounds, on every forward kernel"""
    dtype, C, groups, dg, Cout, knobs = EDGE_INSTANCES[name]
    assert name.startswith(_forward_kernel(dtype, C, groups, dg, Cout, knobs) + "-"), "the case no longer selects the kernel it is named after"
    B, H, W, k, s, p, d = 2, 9, 12, (3, 2), (1, 2), (2, 1), (1, 1)
    x, w, _, mask, bias, _ = _problem(B, C, H, W, Cout, k, s, p, d, groups, dg, dtype, seed=80)
    off = dcn_ref.edge_offsets(B, H, W, k, s, p, d, dg, far=70000 if dtype == torch.float32 else 60000).to(dtype).float()
    assert bool(torch.isfinite(off).all())
    rows, _ = dcn_ref.tap_base(H, W, k, s, p, d)
    y = rows + off.double().view(B, dg, 6, 2, *rows.shape[1:])[:, :, :, 0]
    for edge in (-1.0, -0.5, 0.0, H - 1.0, H - 0.5, float(H)):
        assert bool((y == edge).any()), "the offsets of this dtype no longer put a sample at row %g" % edge
    assert float(y.max()) > 50000 and float(y.min()) < -50000
    dev = lambda t: t.to(DEV).to(dtype)
    with ops.tuning(knobs):
        got1 = dcn.deform_conv(dev(x), dev(off), dev(w), s, p, d, groups, dg)
        got2 = _v2_forward_c(dev(x), dev(off), dev(mask), dev(w), dev(bias), s, p, d, groups, dg)
    want1 = dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg)
    assert float(want1.abs().max()) > 0.1                       # not everything was sampled off the image
    _out_close(got1, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg), "float64": want1}, dtype, "v1")
    _out_close(got2, {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias),
                      "float64": dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)}, dtype, "v2")


# ---- im2col_step ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W,with_weight_grad", [(4, 7, True), (12, 10, False)], ids=["32_output_pixels", "240_output_pixels"])
def test_im2col_step_changes_nothing(H, W, with_weight_grad):
    """B = 4 at steps 1, 2, 4 and 64 (the default: the whole batch): the forward, backward_input (grad_input, grad_offset) and backward_parameters
    (grad_weight) give the bits of step 64.  The reference's step decides how many images share a column buffer; here no such buffer exists.
    grad_weight is compared where it is reproducible at all: its partial sums over ranges of 16 pixels meet in fp32 atomics, and with 32 output
    pixels there are two per element, whose sum does not depend on the order.  Each image is one col2im tile and the offsets stay inside its halo of 4
    pixels, so a cell of grad_input receives one add."""
    k, s, p, d, groups, dg = (3, 2), (1, 2), (0, 1), (1, 1), 2, 2
    x, w, off, _, _, gy = _problem(4, 8, H, W, 6, k, s, p, d, groups, dg, torch.float32, seed=90, off_scale=1.0)
    off = off.clamp(-3.0, 3.0)
    results = {}
    for step in (64, 1, 2, 4):
        xi, oi, wi = (t.to(DEV).requires_grad_() for t in (x, off, w))
        if not with_weight_grad:
            wi = wi.detach()
        y = dcn.deform_conv(xi, oi, wi, s, p, d, groups, dg, step)
        y.backward(gy.to(DEV))
        results[step] = [y.detach(), xi.grad, oi.grad] + ([wi.grad] if with_weight_grad else [])
    _out_close(results[64][0], {"oracle": dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg)}, torch.float32, "forward")
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg)
    for name, g in zip(("input", "offset", "weight"), results[64][1:]):
        _grad_close(g, want[name], torch.float32, "grad_" + name)
    for step in (1, 2, 4):
        for what, a, b in zip(("output", "grad_input", "grad_offset", "grad_weight"), results[step], results[64]):
            assert torch.equal(a, b), "%s at im2col_step %d differs from step 64" % (what, step)


def test_im2col_step_that_does_not_divide_the_batch_is_refused():
    """B = 4, step 3: refused by the Python layer as the reference's does (AssertionError) and by the argument checks of the three v1 entry points (nothing is launched)"""
    k, s, p, d, groups, dg = (3, 2), (1, 2), (0, 1), (1, 1), 2, 2
    x, w, off, _, _, gy = (t.to(DEV) for t in _problem(4, 8, 4, 7, 6, k, s, p, d, groups, dg, torch.float32, seed=90))
    with pytest.raises(AssertionError):
        dcn.deform_conv(x, off, w, s, p, d, groups, dg, 3)
    lib = _lib.load()
    out, gi, go, gw = torch.zeros_like(gy), torch.zeros_like(x), torch.zeros_like(off), torch.zeros_like(w)
    geom = (4, 8, 4, 7, 6, k[1], k[0], s[1], s[0], p[1], p[0], d[1], d[0], groups, dg)
    nf = int(lib.cfen_deform_conv_columns_bytes(0, 4, 8, 4, 7, 6, k[0], k[1], groups))
    nb = int(lib.cfen_deform_conv_backward_bytes(4, 8, 4, 7, 6, k[0], k[1], gy.shape[2], gy.shape[3], groups))
    columns = torch.empty(max(nf, nb), dtype=torch.uint8, device=DEV)
    for step, ok in ((3, False), (2, True)):
        rcs = [lib.cfen_deform_conv_forward(0, ptr(x), ptr(w), ptr(off), ptr(out), *geom, step, ptr(columns), nf, current_stream()),
               lib.cfen_deform_conv_backward_input(0, ptr(x), ptr(off), ptr(gy), ptr(gi), ptr(go), ptr(w), *geom, step, ptr(columns), nb, current_stream()),
               lib.cfen_deform_conv_backward_parameters(0, ptr(x), ptr(off), ptr(gy), ptr(gw), *geom, 1.0, step, ptr(columns), nb, current_stream())]
        assert all((rc == 0) == ok for rc in rcs), (step, rcs)
        if not ok:
            assert b"im2col step must divide batchsize" in lib.cfen_last_error()
    torch.cuda.synchronize()
    assert not out.eq(0).all() and torch.isfinite(gi).all()    # step 2 ran


# ---- backward breadth -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("C,H,dg", [(24, 256, 1), (24, 256, 8), (48, 128, 1), (48, 128, 8), (96, 64, 1), (96, 64, 8)])
def test_deform_conv_backward_at_the_generator_feature_map_shapes(dtype, C, H, dg):
    """(1, 24, 256, 256) / (1, 48, 128, 128) / (1, 96, 64, 64), 3x3 s1 p1, deformable groups 1 and 8, v1 and v2, all gradients against the oracle"""
    geom = (1, C, H, H, C, (3, 3), (1, 1), (1, 1), (1, 1), 1, dg)
    x, w, off, mask, bias, gy = _problem(*geom, dtype, seed=100, off_scale=1.5)
    dev = lambda t: t.to(DEV).to(dtype)
    leaf = lambda t: dev(t).requires_grad_()
    xi, oi, wi = leaf(x), leaf(off), leaf(w)
    dcn.deform_conv(xi, oi, wi, 1, 1, 1, 1, dg).backward(dev(gy))
    _grads_close({"input": xi.grad, "offset": oi.grad, "weight": wi.grad}, {"oracle": dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, 1, dg)}, dtype, "v1")
    xi, oi, mi, wi, bi = leaf(x), leaf(off), leaf(mask), leaf(w), leaf(bias)
    dcn.modulated_deform_conv(xi, oi, mi, wi, bi, 1, 1, 1, 1, dg).backward(dev(gy))
    _grads_close({"input": xi.grad, "offset": oi.grad, "mask": mi.grad, "weight": wi.grad, "bias": bi.grad},
                 {"oracle": dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, 1, dg, mask=mask, with_bias=True)}, dtype, "v2")


def test_deform_conv_backward_refuses_more_output_channels_per_group_than_its_weight_pass_holds():
    """k_dcnb_weight keeps DB_MAXOT = 8 tiles of 16 output channels per wave: 144 output channels per group are refused by the argument check of
    the backward (nothing of it is launched); the forward serves them, and 128 per group pass"""
    for cout, ok in ((288, False), (256, True)):
        x, w, off, _, _, gy = _problem(1, 8, 6, 7, cout, (3, 2), (1, 2), (1, 0), (1, 1), 2, 2, torch.float32, seed=110)
        xi, wi = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
        y = dcn.deform_conv(xi, off.to(DEV), wi, (1, 2), (1, 0), (1, 1), 2, 2)
        _out_close(y.detach(), {"oracle": dcn_oracle.deform_conv(x, off, w, (1, 2), (1, 0), (1, 1), 2, 2)}, torch.float32, "forward")
        if ok:
            y.backward(gy.to(DEV))
            want = dcn_oracle.deform_conv_backward(x, off, w, gy, (1, 2), (1, 0), (1, 1), 2, 2)
            _grads_close({"input": xi.grad, "weight": wi.grad}, {"oracle": want}, torch.float32, "128 per group")
        else:
            with pytest.raises(RuntimeError, match="more than 128 output channels per group"):
                y.backward(gy.to(DEV))


@pytest.mark.parametrize("stride,dilation", [((1, 2), (1, 1)), ((1, 1), (2, 1))], ids=["s12_flushed_tiles", "s11_d21_parked_tiles"])
def test_deform_conv_backward_lds_switch_on_geometry_that_tells_h_from_w(stride, dilation):
    """grad_input (and the rest) with the col2im tiles parked (1), flushed by global atomics (2) and without them (0), 3 x 2 kernel, padding (2, 1):
    at stride (1, 2) a tile's footprint (42 pixels a side) is too large to park, so 1 flushes as 2 does; at stride 1 with dilation (2, 1) it is 29 a side
    and k_dcnb_gin_out gathers the parked tiles -- a tile origin or pitch taken from the wrong axis shows in either"""
    B, C, Cout, k, p, groups, dg = 1, 48, 80, (3, 2), (2, 1), 2, 4
    x, w, off, mask, bias, gy = _problem(B, C, 40, 45, Cout, k, stride, p, dilation, groups, dg, torch.float32, seed=120, off_scale=3.0)
    s, d = stride, dilation
    want = dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg, mask=mask, with_bias=True)
    lib = _lib.load()
    dev = lambda t: t.to(DEV)
    for lds in (1, 2, 0):
        old = lib.cfen_deform_conv_backward_set_lds(lds)
        try:
            got = _v2_backward_c(dev(x), dev(off), dev(mask), dev(w), dev(gy), s, p, d, groups, dg)
            xi = dev(x).requires_grad_()
            dcn.deform_conv(xi, dev(off), dev(w), s, p, d, groups, dg).backward(dev(gy))
            torch.cuda.synchronize()
        finally:
            lib.cfen_deform_conv_backward_set_lds(old)
        _grads_close(got, {"oracle": want}, torch.float32, "v2 (lds=%d)" % lds)
        _grad_close(xi.grad, dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg)["input"], torch.float32, "v1 grad_input (lds=%d)" % lds)
