"""The yardstick of the padded-row LayerNorm (include/cfen_padnorm.h), CPU only: value_edges_ref's rows scattered into the padded token layout of the
v5 LViT blocks, the float64 reference and the e32 of its bar over the real slots, and fp32 restatements of the kernel's own arithmetic -- the
correction formula k_layernorm had for padded rows, and the masked one it has now.  test_padnorm_host.py checks the yardstick and both
restatements; test_hip_value_edges.py and test_hip_ops.py hold the kernel to it.

Layout: a row is PP pixels of cs slots, slot s is real iff s % cs < C; real entry r of a row sits in slot (r // C) * cs + r % C."""
import torch

import value_edges_ref as ve

PP = 4                              # p * p of the LViT blocks
LAYOUTS = ((8, 6), (16, 12))        # (cs, C) of v5 levels 1 and 2 at n_feats 24; level 3 (24, 24) has no padding


def dims(cs, C):
    """(D, Dn)"""
    return PP * cs, PP * C


def real_slots(cs, C, D=None):
    D = PP * cs if D is None else D
    return torch.arange(D) % cs < C


def scatter(real, cs, C, fill=0.0):
    """(..., Dn) -> (..., D): the real entries in their slots, `fill` in the padding slots"""
    D = real.shape[-1] // C * cs
    out = torch.full(real.shape[:-1] + (D,), fill, dtype=real.dtype)
    out[..., real_slots(cs, C, D)] = real
    return out


def rows(case, M, cs, C, dtype, seed=0):
    """value_edges_ref.rows of the case over the Dn real entries, in the padded layout (padding slots exact zeros)"""
    return scatter(ve.rows(case, M, PP * C, dtype, seed), cs, C)


def ln_operands(cs, C, seed=0):
    """gamma, beta of the padded row: zero in the padding slots, as packing.pack_vit_shrunk delivers them"""
    g, b = ve.ln_operands(PP * C, seed)
    return scatter(g, cs, C), scatter(b, cs, C)


def layernorm(x, g, b, cs, C, cdt, eps=1e-5):
    """the definition in precision cdt: value_edges_ref.layernorm (centred two-pass) over the real slots, beta in the others"""
    m = real_slots(cs, C, x.shape[-1])
    out = b.to(cdt).expand(x.shape).clone()
    out[..., m] = ve.layernorm(x[..., m], g[m], b[m], cdt, eps=eps)
    return out


def _group_sum(lane):
    """(M, G) per-lane partial sums -> (M,): the butterfly of the kernel's lane group, neighbours first, in fp32"""
    while lane.shape[-1] > 1:
        lane = lane[..., 0::2] + lane[..., 1::2]
    return lane[..., 0]


def kernel_restated(x, g, b, cs, C, formula, eps=1e-5):
    """k_layernorm's arithmetic for rows of up to 16 vectors (one 16-byte vector of x's dtype per lane, 16 lanes per row) in float32: the row held as
    v - p with p its first element, one running sum per lane, the lanes summed pairwise.
    formula "correction": every slot centred to v - p, the (D - Dn) zero slots taken back out of both sums afterwards (the kernel before
    include/cfen_padnorm.h); "masked": a padding slot is 0 after centring in both passes and no correction exists (the kernel now)."""
    f32 = torch.float32
    M, D = x.shape
    epl = 16 // x.element_size()
    nvec = D // epl
    assert D % epl == 0 and nvec <= 16
    Dn = D // cs * C
    real = real_slots(cs, C, D)
    masked = {"masked": True, "correction": False}[formula]
    xf = x.to(f32)
    p = xf[:, :1]
    v = xf - p
    if masked:
        v = torch.where(real, v, torch.zeros((), dtype=f32))

    def lanes(t):                                     # running sum over the elements of a lane's vector, idle lanes hold 0
        t = t.view(M, nvec, epl)
        acc = torch.zeros(M, nvec, dtype=f32)
        for e in range(epl):
            acc = acc + t[:, :, e]
        return _group_sum(torch.cat([acc, torch.zeros(M, 16 - nvec, dtype=f32)], 1))
    s = lanes(v)
    if not masked:
        s = s + torch.tensor(float(D - Dn), dtype=f32) * p[:, 0]
    mean = (s / torch.tensor(float(Dn), dtype=f32)).view(M, 1)
    d = v - mean
    if masked:
        d = torch.where(real, d, torch.zeros((), dtype=f32))
    sq = lanes(d * d)
    if not masked:
        pm = p[:, 0] + mean[:, 0]
        sq = sq - torch.tensor(float(D - Dn), dtype=f32) * pm * pm
    rstd = torch.rsqrt(sq.clamp_min(0) / torch.tensor(float(Dn), dtype=f32) + torch.tensor(eps, dtype=f32)).view(M, 1)
    return d * rstd * g.to(f32) + b.to(f32)


def yardstick(case, M, cs, C, dtype):
    """(x, gamma, beta, want, e32): the padded rows of the case, the float64 reference, and the max-abs distance from it of the centred two-pass
    fp32 restatement over the real slots"""
    x = rows(case, M, cs, C, dtype)
    g, b = ln_operands(cs, C)
    want = layernorm(x, g, b, cs, C, torch.float64)
    return x, g, b, want, ve.e32_of(layernorm(x, g, b, cs, C, torch.float32), want)
