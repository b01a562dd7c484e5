"""Pin the C oracle of the deformable conv (oracle/dcn_oracle.c): with the known-answer properties that
follow from the reference kernel code, and element by element -- the output and all five
gradients -- against tests/dcn_ref.py, a float64 restatement of the operator's definition whose gradients
come from autograd (nothing in it is hand-derived, so it shares no code and no derivation with the oracle or
the kernels).  The reference ships no DCN tests or vectors and its CUDA extension cannot be built here, so
parity against the reference's own binary stays unpinned (stated in the oracle's header).

Worst oracle <-> float64 max-abs distances measured over the six h/w-distinct geometries of GEOMETRIES, v1 and
v2 (bar: 1e-5 x max(1, |want|max); each test prints its own):
  output 2.7e-6, grad_input 2.0e-6, grad_offset 4.4e-6, grad_mask 3.1e-6, grad_weight 8.8e-6 (where |want|max
  is 16.5: 5.4e-7 of it), grad_bias 5.7e-7; at the edge sample positions (forward only): output 1.5e-7.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import dcn_oracle
import dcn_ref


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("k,stride,pad,dil,groups", [(3, 1, 1, 1, 1), (3, 2, 1, 1, 1), (3, 1, 2, 2, 1), (5, 1, 2, 1, 2), (1, 1, 0, 1, 1)])
def test_zero_offsets_equal_conv2d(k, stride, pad, dil, groups):
    # integer sample points give bilinear weights (1,0,0,0); the (-1,H) bound reproduces zero padding (.cu:226-236)
    x, w = rnd((2, 8, 11, 13), 1), rnd((6, 8 // groups, k, k), 2, 0.2)
    want = F.conv2d(x, w, None, stride, pad, dil, groups)
    off = torch.zeros(2, 2 * k * k, want.shape[2], want.shape[3])
    got = dcn_oracle.deform_conv(x, off, w, stride, pad, dil, groups, 1)
    assert torch.allclose(got, want, atol=1e-5)


def test_integer_offsets_equal_shifted_taps():
    x, w = rnd((1, 4, 12, 12), 3), rnd((5, 4, 3, 3), 4, 0.3)
    off = torch.zeros(1, 18, 12, 12)
    off[:, 0::2] = 2.0          # every tap samples 2 rows lower
    off[:, 1::2] = -1.0         # and 1 column to the left
    got = dcn_oracle.deform_conv(x, off, w, 1, 1, 1, 1, 1)
    xs = torch.zeros(1, 4, 12 + 8, 12 + 8)
    xs[:, :, 4:16, 4:16] = x
    # shifted image with zeros outside: out(y,x) = conv(x_shift), x_shift(y,x) = x(y+2, x-1)
    x_shift = xs[:, :, 6:18, 3:15]
    want = F.conv2d(x_shift, w, padding=1)
    # taps that land outside the ORIGINAL image are zero in both; but conv's own zero padding ring of
    # x_shift differs from sampling x beyond the ring -> compare the interior that does not touch it
    assert torch.allclose(got[:, :, 1:-1, 1:-1], want[:, :, 1:-1, 1:-1], atol=1e-5)


def test_fractional_offsets_interpolate():
    # single channel, 1x1 kernel, weight 1: the op IS bilinear sampling
    x = torch.arange(25, dtype=torch.float32).view(1, 1, 5, 5)
    off = torch.zeros(1, 2, 5, 5)
    off[:, 0], off[:, 1] = 0.5, 0.25
    got = dcn_oracle.deform_conv(x, off, torch.ones(1, 1, 1, 1), 1, 0, 1, 1, 1)
    # interior: value + 0.5*5 + 0.25*1
    assert torch.allclose(got[0, 0, :4, :4], x[0, 0, :4, :4] + 2.75, atol=1e-5)
    # last row samples h=4.5: rows 4 and 5(out of range -> 0): half weight
    assert torch.allclose(got[0, 0, 4, :4], 0.5 * (x[0, 0, 4, :4] * 0.75 + x[0, 0, 4, 1:5] * 0.25), atol=1e-5)


def test_mask_one_equals_v1_plus_bias_and_mask_scales():
    x, w, b = rnd((2, 6, 9, 9), 5), rnd((4, 6, 3, 3), 6, 0.2), rnd((4,), 7)
    off = rnd((2, 2 * 2 * 9, 9, 9), 8, 1.5)                      # deformable_groups = 2
    v1 = dcn_oracle.deform_conv(x, off, w, 1, 1, 1, 1, 2)
    v2 = dcn_oracle.deform_conv(x, off, w, 1, 1, 1, 1, 2, mask=torch.ones(2, 2 * 9, 9, 9), bias=b)
    assert torch.allclose(v2, v1 + b.view(1, -1, 1, 1), atol=1e-5)
    half = dcn_oracle.deform_conv(x, off, w, 1, 1, 1, 1, 2, mask=torch.full((2, 18, 9, 9), 0.5))
    assert torch.allclose(half, 0.5 * v1, atol=1e-5)


def test_deformable_groups_use_their_own_offsets():
    x, w = rnd((1, 4, 8, 8), 9), rnd((3, 4, 3, 3), 10, 0.3)
    off = torch.zeros(1, 2 * 18, 8, 8)
    off[:, 18:] = 1.0                                            # second group (channels 2,3) shifted by (+1,+1)
    got = dcn_oracle.deform_conv(x, off, w, 1, 1, 1, 1, 2)
    a = dcn_oracle.deform_conv(x[:, :2], torch.zeros(1, 18, 8, 8), w[:, :2].contiguous(), 1, 1, 1, 1, 1)
    b = dcn_oracle.deform_conv(x[:, 2:], torch.ones(1, 18, 8, 8), w[:, 2:].contiguous(), 1, 1, 1, 1, 1)
    assert torch.allclose(got, a + b, atol=1e-5)


def test_invalid_shapes_rejected():
    with pytest.raises(ValueError):
        dcn_oracle.deform_conv(torch.zeros(1, 3, 2, 2), torch.zeros(1, 18, 1, 1), torch.zeros(2, 3, 3, 3), 1, 0, 1, 1, 1)


# ---- backward (oracle/dcn_oracle.c: dcn_oracle_backward) -------------------------------------------------------------------------------

@pytest.mark.parametrize("k,stride,pad,dil,groups", [(3, 1, 1, 1, 1), (3, 2, 1, 1, 1), (3, 1, 2, 2, 2), (1, 1, 0, 1, 1)])
def test_backward_at_zero_offsets_equals_conv2d_autograd(k, stride, pad, dil, groups):
    x, w, b = rnd((2, 8, 9, 10), 1).requires_grad_(), rnd((6, 8 // groups, k, k), 2, 0.2).requires_grad_(), rnd((6,), 3).requires_grad_()
    y = F.conv2d(x, w, b, stride, pad, dil, groups)
    gy = rnd(tuple(y.shape), 4)
    y.backward(gy)
    off = torch.zeros(2, 2 * k * k, y.shape[2], y.shape[3])
    mask = torch.ones(2, k * k, y.shape[2], y.shape[3])
    for m in (None, mask):
        g = dcn_oracle.deform_conv_backward(x.detach(), off, w.detach(), gy, stride, pad, dil, groups, 1, mask=m, with_bias=True)
        assert torch.allclose(g["input"], x.grad, atol=2e-5)
        assert torch.allclose(g["weight"], w.grad, atol=2e-4)
        assert torch.allclose(g["bias"], b.grad, atol=2e-4)


@pytest.mark.parametrize("dg,groups,with_mask", [(1, 1, False), (2, 1, True), (4, 2, True)])
def test_backward_matches_finite_differences_of_the_forward_oracle(dg, groups, with_mask):
    """d loss / d offset, d loss / d mask, d loss / d input, d loss / d weight of loss = <forward, grad_out>, against central differences of
    dcn_oracle.deform_conv (itself pinned above).  Offsets are kept away from integer sample positions, where the bilinear sample has a kink."""
    B, C, H, W, Cout, k = 1, 8, 7, 6, 4, 3
    x, w = rnd((B, C, H, W), 11), rnd((Cout, C // groups, k, k), 12, 0.3)
    g = torch.Generator().manual_seed(13)
    off = (torch.rand(B, dg * 2 * k * k, H, W, generator=g) * 0.6 + 0.2) * (torch.randint(0, 2, (B, dg * 2 * k * k, H, W), generator=g) * 2 - 1) * 1.3
    frac = off - off.floor()
    off = torch.where((frac < 0.1) | (frac > 0.9), off.floor() + 0.5, off)
    mask = torch.rand(B, dg * k * k, H, W, generator=g) if with_mask else None
    gy = rnd((B, Cout, H, W), 14)
    fwd = lambda x_, off_, w_, m_: float((dcn_oracle.deform_conv(x_, off_, w_, 1, 1, 1, groups, dg, mask=m_).double() * gy.double()).sum())
    got = dcn_oracle.deform_conv_backward(x, off, w, gy, 1, 1, 1, groups, dg, mask=mask)
    eps = 1e-2
    picks = torch.randperm(off.numel(), generator=g)[:40]
    for idx in picks.tolist():
        d = torch.zeros(off.numel()); d[idx] = eps
        d = d.view_as(off)
        num = (fwd(x, off + d, w, mask) - fwd(x, off - d, w, mask)) / (2 * eps)
        assert abs(num - float(got["offset"].flatten()[idx])) <= 2e-3 * max(1.0, abs(num)), (idx, num, float(got["offset"].flatten()[idx]))
    for name, t in (("input", x), ("weight", w)) + ((("mask", mask),) if with_mask else ()):
        for idx in torch.randperm(t.numel(), generator=g)[:25].tolist():
            d = torch.zeros(t.numel()); d[idx] = eps
            d = d.view_as(t)
            def at(sign):
                if name == "input":
                    return fwd(x + sign * d, off, w, mask)
                if name == "weight":
                    return fwd(x, off, w + sign * d, mask)
                return fwd(x, off, w, mask + sign * d)
            num = (at(1) - at(-1)) / (2 * eps)                      # the forward is linear in each of these: exact up to fp32 rounding
            assert abs(num - float(got[name].flatten()[idx])) <= 2e-3 * max(1.0, abs(num)), (name, idx)


def test_backward_is_linear_in_grad_output_and_accumulates_weight_grads():
    x, w = rnd((2, 4, 6, 6), 21), rnd((4, 4, 3, 3), 22, 0.3)
    off, mask = rnd((2, 18, 6, 6), 23, 0.7), torch.rand(2, 9, 6, 6, generator=torch.Generator().manual_seed(24))
    g1, g2 = rnd((2, 4, 6, 6), 25), rnd((2, 4, 6, 6), 26)
    a = dcn_oracle.deform_conv_backward(x, off, w, g1, 1, 1, 1, 1, 1, mask=mask, with_bias=True)
    b = dcn_oracle.deform_conv_backward(x, off, w, g2, 1, 1, 1, 1, 1, mask=mask, with_bias=True)
    c = dcn_oracle.deform_conv_backward(x, off, w, g1 * 2 - g2, 1, 1, 1, 1, 1, mask=mask, with_bias=True)
    for k in a:
        assert torch.allclose(c[k], 2 * a[k] - b[k], atol=1e-4), k
    half = dcn_oracle.deform_conv_backward(x, off, w, g1, 1, 1, 1, 1, 1, mask=mask, scale=0.5)
    assert torch.allclose(half["weight"], 0.5 * a["weight"], atol=1e-5)       # deform_conv_backward_parameters_cuda's `scale`


# ---- the oracle against the float64 autograd restatement (tests/dcn_ref.py), every element ------------------------------------------------

# (B, C, H, W, Cout, (kh, kw), (sh, sw), (ph, pw), (dh, dw), groups, deformable groups): every h / w pair differs somewhere
GEOMETRIES = {
    "1x3_s12_p01_d12_g2_dg2": (2, 8, 9, 11, 6, (1, 3), (1, 2), (0, 1), (1, 2), 2, 2),             # a row kernel
    "3x1_s21_p10_d21_g1_dg3": (2, 6, 10, 8, 4, (3, 1), (2, 1), (1, 0), (2, 1), 1, 3),             # a column kernel
    "3x2_s12_p21_g4_dg2_dg_spans_groups": (2, 8, 9, 12, 8, (3, 2), (1, 2), (2, 1), (1, 1), 4, 2),   # a deformable group of 4 channels over two conv groups of 2
    "5x3_s21_p23_d12_g2_dg6_group_spans_dgs": (2, 12, 11, 9, 6, (5, 3), (2, 1), (2, 3), (1, 2), 2, 6),   # a conv group of 6 channels over three deformable groups of 2
    "2x4_s13_p12_d31_g1_dg8": (3, 8, 8, 13, 4, (2, 4), (1, 3), (1, 2), (3, 1), 1, 8),
    "3x3_s23_p02_d21_g1_dg1": (2, 4, 12, 10, 8, (3, 3), (2, 3), (0, 2), (2, 1), 1, 1),
}
BAR = 1e-5      # x max(1, |want|max): the tolerance of the known-answer pins above


def _far(got, want):
    """(max-abs distance, its bar)"""
    return float((got.double() - want).abs().max()), BAR * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_oracle_equals_float64_autograd_reference_on_every_element(name, modulated):
    """output, grad_input, grad_offset, grad_mask, grad_weight, grad_bias of loss = <output, grad_out>; sample positions kept 0.02 away from
    integer coordinates for the gradients' sake (the bilinear sample has a kink there)"""
    B, C, H, W, Cout, k, s, p, d, groups, dg = GEOMETRIES[name]
    Ho, Wo = dcn_ref.out_size(H, W, k, s, p, d)
    kk = k[0] * k[1]
    x, w = rnd((B, C, H, W), 31), rnd((Cout, C // groups, k[0], k[1]), 32, 0.3)
    off = dcn_ref.keep_off_integers(rnd((B, dg * 2 * kk, Ho, Wo), 33, 1.5))
    mask = torch.rand(B, dg * kk, Ho, Wo, generator=torch.Generator().manual_seed(34)) if modulated else None
    bias = rnd((Cout,), 35) if modulated else None
    gy = rnd((B, Cout, Ho, Wo), 36)
    leaves = {"input": x, "offset": off, "weight": w}
    if modulated:
        leaves.update(mask=mask, bias=bias)
    leaves = {n: t.double().requires_grad_() for n, t in leaves.items()}
    want = dcn_ref.deform_conv_f64(leaves["input"], leaves["offset"], leaves["weight"], s, p, d, groups, dg, mask=leaves.get("mask"), bias=leaves.get("bias"))
    want.backward(gy.double())
    got = dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)
    grads = dcn_oracle.deform_conv_backward(x, off, w, gy, s, p, d, groups, dg, mask=mask, with_bias=modulated)
    assert got.shape == want.shape
    report, failed = [], []
    for what, g, r in [("output", got, want.detach())] + [("grad_" + n, grads[n], t.grad) for n, t in leaves.items()]:
        dist, bar = _far(g, r)
        report.append("%s %.2e (|want|max %.1f)" % (what, dist, float(r.abs().max())))
        if not dist <= bar:
            failed.append("%s: %.3e > %.1e" % (what, dist, bar))
    print("oracle <-> float64 [%s %s]: %s" % (name, "v2" if modulated else "v1", ", ".join(report)))
    assert not failed, failed


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("name", ["3x2_s12_p21_g4_dg2_dg_spans_groups", "3x3_s23_p02_d21_g1_dg1"])
def test_oracle_equals_float64_reference_at_the_edge_sample_positions(name, modulated):
    """forward only: samples exactly at -1, -0.5, 0, n - 1, n - 0.5 and n per axis, at integer positions, and 70 000 pixels off the image"""
    B, C, H, W, Cout, k, s, p, d, groups, dg = GEOMETRIES[name]
    Ho, Wo = dcn_ref.out_size(H, W, k, s, p, d)
    kk = k[0] * k[1]
    x, w = rnd((B, C, H, W), 41), rnd((Cout, C // groups, k[0], k[1]), 42, 0.3)
    off = dcn_ref.edge_offsets(B, H, W, k, s, p, d, dg, far=70000).float()
    rows, cols = dcn_ref.tap_base(H, W, k, s, p, d)
    y = rows + off.double().view(B, dg, kk, 2, Ho, Wo)[:, :, :, 0]
    for edge in (-1.0, -0.5, 0.0, H - 1.0, H - 0.5, float(H), -70000.0, 70000.0):
        assert bool((y == edge).any()), "float32 offsets no longer put a sample at row %g" % edge
    mask = torch.rand(B, dg * kk, Ho, Wo, generator=torch.Generator().manual_seed(44)) if modulated else None
    bias = rnd((Cout,), 45) if modulated else None
    want = dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)
    got = dcn_oracle.deform_conv(x, off, w, s, p, d, groups, dg, mask=mask, bias=bias)
    dist, bar = _far(got, want)
    print("oracle <-> float64 at the edges [%s %s]: output %.2e" % (name, "v2" if modulated else "v1", dist))
    assert dist <= bar
    assert float(want.abs().max()) > 0.1                       # not everything was sampled off the image
