"""Float64 restatement of the deformable convolution (DCNv1, and DCNv2 with a mask and a bias) in plain torch, differentiable by autograd.

Written from the operator's definition (header of oracle/dcn_oracle.c), not from anybody's loops, and with no hand-derived gradient:
  * offset channels are laid out (deformable group, tap = i * kw + j, [dy, dx], Ho, Wo);
  * tap (i, j) of output pixel (ho, wo) samples every channel of its deformable group at
    (ho * sh - ph + i * dh + dy,  wo * sw - pw + j * dw + dx);
  * the sample is bilinear over the four pixels around that point, and a corner outside [0, H) x [0, W) contributes zero (which makes a sample
    at or beyond -1 / H / W zero as a whole);
  * the sample is multiplied by the tap's mask when there is one;
  * the samples are contracted with the weights per convolution group, and the bias is added.
It pins oracle/dcn_oracle.c (tests/test_dcn_oracle.py) and, where a case is small enough, the HIP kernels directly (tests/test_hip_dcn.py)."""
import torch


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def out_size(H, W, kernel, stride, padding, dilation):
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    return (H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1, (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1


def tap_base(H, W, kernel, stride, padding, dilation):
    """the undeformed sample positions: two (kh * kw, Ho, Wo) float64 tensors of rows and columns"""
    (kh, kw), (sh, sw), (ph, pw), (dh, dw) = _pair(kernel), _pair(stride), _pair(padding), _pair(dilation)
    Ho, Wo = out_size(H, W, kernel, stride, padding, dilation)
    i = torch.arange(kh, dtype=torch.float64).repeat_interleave(kw)
    j = torch.arange(kw, dtype=torch.float64).repeat(kh)
    rows = (torch.arange(Ho, dtype=torch.float64) * sh - ph).view(1, Ho, 1) + (i * dh).view(-1, 1, 1)
    cols = (torch.arange(Wo, dtype=torch.float64) * sw - pw).view(1, 1, Wo) + (j * dw).view(-1, 1, 1)
    return rows.expand(kh * kw, Ho, Wo), cols.expand(kh * kw, Ho, Wo)


def deform_conv_f64(x, offset, weight, stride, padding, dilation, groups, deformable_groups, mask=None, bias=None):
    x, offset, weight = x.double(), offset.double(), weight.double()
    B, C, H, W = x.shape
    Cout, Cg, kh, kw = weight.shape
    dg, kk = deformable_groups, kh * kw
    assert C == Cg * groups and Cout % groups == 0 and C % dg == 0
    Ho, Wo = out_size(H, W, (kh, kw), stride, padding, dilation)
    assert Ho >= 1 and Wo >= 1 and tuple(offset.shape) == (B, dg * 2 * kk, Ho, Wo)
    rows, cols = tap_base(H, W, (kh, kw), stride, padding, dilation)
    off = offset.view(B, dg, kk, 2, Ho, Wo)
    y, xx = rows + off[:, :, :, 0], cols + off[:, :, :, 1]                        # (B, dg, kk, Ho, Wo)
    y0, x0 = y.detach().floor(), xx.detach().floor()
    ly, lx = y - y0, xx - x0
    img = x.reshape(B, dg, C // dg, H * W)
    sample = 0.0
    for yc, wy in ((y0, 1.0 - ly), (y0 + 1.0, ly)):
        for xc, wx in ((x0, 1.0 - lx), (x0 + 1.0, lx)):
            inside = ((yc >= 0) & (yc <= H - 1) & (xc >= 0) & (xc <= W - 1)).double()
            idx = (yc.clamp(0, H - 1) * W + xc.clamp(0, W - 1)).long().view(B, dg, 1, kk * Ho * Wo).expand(B, dg, C // dg, kk * Ho * Wo)
            corner = torch.gather(img, 3, idx).view(B, dg, C // dg, kk, Ho, Wo)
            sample = sample + corner * (wy * wx * inside).unsqueeze(2)
    if mask is not None:
        sample = sample * mask.double().view(B, dg, 1, kk, Ho, Wo)
    out = torch.einsum("bgckhw,gock->bgohw", sample.reshape(B, groups, Cg, kk, Ho, Wo), weight.view(groups, Cout // groups, Cg, kk))
    out = out.reshape(B, Cout, Ho, Wo)
    return out if bias is None else out + bias.double().view(1, Cout, 1, 1)


def keep_off_integers(offset, margin=0.02):
    """move every offset's fractional part into [margin, 1 - margin]: stride, padding and dilation are integers, so the sample positions then stay
    `margin` away from integer coordinates, where the bilinear sample has a kink and a gradient is a matter of convention"""
    fl = offset.floor()
    return fl + margin + (offset - fl) * (1.0 - 2.0 * margin)


def edge_offsets(B, H, W, kernel, stride, padding, dilation, deformable_groups, far):
    """Offsets (float64) that put the samples ON the operator's edges: per axis exactly -1, -0.5, 0, n - 1, n - 0.5 and n (n = H or W), an
    interior integer, two interior fractions, and `far` pixels to either side of the image; every pair (row position, column position) occurs."""
    def positions(n):
        return [-1.0, -0.5, 0.0, n - 1.0, n - 0.5, float(n), float(min(2, n - 1)), 0.25 * n, n - 1.25, -float(far), float(far)]
    rows, cols = tap_base(H, W, kernel, stride, padding, dilation)
    kk, Ho, Wo = rows.shape
    py, px = positions(H), positions(W)
    n = torch.arange(B * deformable_groups * kk * Ho * Wo).view(B, deformable_groups, kk, Ho, Wo)
    assert n.numel() >= len(py) * len(px), "too few samples for every pair of edge positions"
    ty = torch.tensor(py, dtype=torch.float64)[n % len(py)]
    tx = torch.tensor(px, dtype=torch.float64)[(n // len(py)) % len(px)]
    return torch.stack((ty - rows, tx - cols), dim=3).reshape(B, deformable_groups * 2 * kk, Ho, Wo)
