"""Inputs, float64 references and bars of the value-edge tests (CPU only; test_value_edges_host.py checks this yardstick itself,
test_hip_value_edges.py holds the kernels to it).

The rest of the suite feeds every normalising kernel rows / channels whose mean is about their spread.  Here the mean is rho times the spread:
rho in RHOS, plus a row whose variance is near eps, an exactly constant row and rows whose mean alternates in sign.  At rho = 256 a variance formed
as E[x^2] - mean^2 from fp32 sums has lost every bit of a unit variance; one formed from centred values has lost none.

Bar of an output element:  |got - want| <= BAR_FACTOR * e32 + (2^-10 |want| for fp16 outputs),  e32 = the max-abs distance from float64 of an fp32
restatement of the same operation with centred (two-pass) statistics, on the same operands.  Nothing in the bar comes from a kernel's result.
4 = another summation order than the restatement's + the scatter of a maximum over a few thousand elements; 2^-10 = one fp16 output rounding
(2^-11) and a double-rounding slip."""
import math

import torch

from cfen_vit_dehazing_amd import packing

RHOS = (0, 1, 8, 64, 256)
CASES = tuple("rho%d" % r for r in RHOS) + ("tiny_std", "constant", "alt_sign")
BAR_FACTOR = 4.0
F16_OUT = 2.0 ** -10
ALT_RHO = 64.0          # |mean| of the alternating-sign case


# ---------------------------------------------------------------------------------------------------
# input builders
def _unit(shape, seed):
    """seeded normal samples, standardised along the last axis: mean exactly 0 and (biased) std exactly 1 in float64"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(shape, generator=g, dtype=torch.float64)
    z = z - z.mean(-1, keepdim=True)
    return z / z.pow(2).mean(-1, keepdim=True).sqrt()


def rows(case, M, D, dtype, seed=0):
    """(M, D) matrix of the dtype under test, every row of the named case (rounded to dtype here: reference and kernel see the same operands)"""
    z = _unit((M, D), 1000 + seed)
    if case.startswith("rho"):
        x = z + float(case[3:])
    elif case == "tiny_std":
        x = 1e-2 * z + 1.0                                      # rho = 100, variance 1e-4 against eps = 1e-5
    elif case == "constant":
        # a dyadic constant per row: every partial sum of copies of it is exact in fp32 in any order, so the exact answer (beta, or 0) is
        # reachable and e32 = 0 is a fair bar; any other constant would leave the bar to the luck of the restatement's own summation order
        x = (0.25 * (1 + torch.arange(M, dtype=torch.float64) % 16)).view(M, 1).expand(M, D).clone()
    elif case == "alt_sign":
        sign = 1.0 - 2.0 * (torch.arange(M, dtype=torch.float64) % 2)
        x = z + ALT_RHO * sign.view(M, 1)
    else:
        raise KeyError(case)
    return x.to(dtype)


def channels(B, C, H, W, dtype, seed=0):
    """(B, C, H, W) map: channel c is case CASES[c % len(CASES)] over its H * W pixels; alt_sign alternates along the batch.
    Returns (x, [case name per channel])."""
    names = [CASES[c % len(CASES)] for c in range(C)]
    x = torch.empty(B, C, H, W, dtype=torch.float64)
    for c, nm in enumerate(names):
        r = rows(nm, B, H * W, torch.float64, seed=seed + 17 * c)
        if nm == "constant":
            r = torch.full((B, H * W), 0.25 * (1 + c % 16), dtype=torch.float64)
        x[:, c] = r.view(B, H, W)
    return x.to(dtype), names


def ln_operands(D, seed=0):
    g = torch.Generator().manual_seed(50 + seed)
    return 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def fold_operands(K, N, dtype, seed=0):
    g = torch.Generator().manual_seed(60 + seed)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    gam, bet = ln_operands(K, seed)
    f = packing.ln_folded(None, gam, bet, torch.randn(N, generator=g), "l", dtype, w)
    return f["l.wl"], f["l.s"], f["l.bl"]


def rho_of(x):
    """|mean| / std along the last axis, float64 (inf for a constant row)"""
    x = x.double()
    mu = x.mean(-1)
    sd = (x - mu.unsqueeze(-1)).pow(2).mean(-1).sqrt()
    return mu.abs() / sd


# ---------------------------------------------------------------------------------------------------
# statistics: centred (two-pass) and one-pass, in the dtype of x
def stats_two_pass(x, dim=-1):
    mu = x.mean(dim, keepdim=True)
    return mu, (x - mu).pow(2).mean(dim, keepdim=True)


def _chunked_sum(v, chunk, finish):
    """sum over the last axis as a kernel forms it: one running sum per chunk of `chunk` consecutive elements in v's own precision (torch.sum
    adds pairwise, which hides most of what a running sum loses), the chunk totals added in `finish`"""
    n = v.shape[-1]
    pad = (-n) % chunk
    if pad:
        v = torch.cat([v, v.new_zeros(v.shape[:-1] + (pad,))], -1)
    v = v.reshape(v.shape[:-1] + (-1, chunk))
    acc = torch.zeros_like(v[..., 0])
    for i in range(chunk):
        acc = acc + v[..., i]
    return acc.to(finish).sum(-1, keepdim=True)


def stats_one_pass(x, dim=-1, chunk=64, finish=None):
    """E[x^2] - mean^2, clamped at 0, from running sums of x and x^2 in x's own precision: the formula the value-edge tests exist to catch.
    finish = torch.float64 models the channel statistics (fp32 partial sums per chunk of pixels, finished in double): the double does not
    bring back what the fp32 sum of squares has already lost."""
    dims = (dim,) if isinstance(dim, int) else tuple(dim)
    flat = x.flatten(min(d % x.dim() for d in dims)) if len(dims) > 1 else x
    fin = finish or x.dtype
    n = flat.shape[-1]
    mu = _chunked_sum(flat, chunk, fin) / n
    var = (_chunked_sum(flat * flat, chunk, fin) / n - mu * mu).clamp_min(0)
    shape = mu.shape[:-1] + (1,) * len(dims)
    return mu.reshape(shape).to(x.dtype), var.reshape(shape).to(x.dtype)


# ---------------------------------------------------------------------------------------------------
# the operations, generic in precision (cdt = torch.float64: the reference; torch.float32: the restatement / the one-pass model)
def layernorm(x, g, b, cdt, stats=stats_two_pass, eps=1e-5):
    x = x.to(cdt)
    mu, var = stats(x)
    return (x - mu) * torch.rsqrt(var + eps) * g.to(cdt) + b.to(cdt)


def gemm_ln(x, wl, s, bl, cdt, stats=stats_two_pass, eps=1e-5, relu=False):
    """the fold's own form on the packed operands: rstd (x wl^T - mean s) + bl; its acc - s mean cancellation belongs to the fold"""
    x = x.to(cdt)
    mu, var = stats(x)
    y = torch.rsqrt(var + eps) * (x @ wl.to(cdt).t() - mu * s.to(cdt)) + bl.to(cdt)
    return y.relu() if relu else y


def instnorm_relu(x, cdt, stats=stats_two_pass, eps=1e-5):
    x = x.to(cdt)
    mu, var = stats(x, (2, 3))
    return ((x - mu) * torch.rsqrt(var + eps)).relu()


def actnorm_init(x, cdt):
    """models/actnorm.py first-call init, centred: (weight, bias) = (-0.5 log max(var_unbiased, 0.2), -mean) over batch and pixels"""
    xt = x.to(cdt).transpose(0, 1).reshape(x.shape[1], -1)
    mu = xt.mean(1, keepdim=True)
    var = (xt - mu).pow(2).sum(1) / (xt.shape[1] - 1)
    return -0.5 * torch.log(var.clamp_min(0.2)), -mu[:, 0]


# ---------------------------------------------------------------------------------------------------
# the bar
def e32_of(restated, want):
    return float((restated.double() - want).abs().max())


def bar(want, e32, out_dtype):
    """per-element bound on |got - want|"""
    b = torch.full_like(want, BAR_FACTOR * e32)
    return b + F16_OUT * want.abs() if out_dtype == torch.float16 else b


def ratio(got, want, e32, out_dtype):
    """worst |got - want| / bar over the elements (an element with bar 0 and no error counts 0; with bar 0 and an error, inf);
    a non-finite result is inf"""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, b = (got - want).abs(), bar(want, e32, out_dtype)
    r = torch.where(err == 0, torch.zeros_like(err), err / b)
    return float(r.max())


# ---------------------------------------------------------------------------------------------------
# softmax
def attn_ref(qkv, nseq, S, heads):
    D = qkv.shape[1] // 3
    dh = D // heads
    q, k, v = qkv.double().view(nseq, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dh), -1) @ v
    return a.transpose(1, 2).reshape(nseq * S, D)


def dominant_positions(S):
    """index 0, S - 1, both sides of every key-block edge of the kernels (128 / 256 keys), and inside the ragged last block of S = 100"""
    return sorted({p for p in (0, S - 1, 127, 128, 255, 256) + ((97,) if S == 100 else ()) if p < S})


def softmax_cases(S, heads, dh, dtype, nseq=2, seed=0):
    """[(name, qkv [nseq * S, 3 * heads * dh] of dtype)]: every value finite and |x| <= ~300"""
    D = heads * dh
    g = torch.Generator().manual_seed(4000 + seed + S)
    base = 0.5 * torch.randn(nseq * S, 3, heads, dh, generator=g, dtype=torch.float64)
    out = []
    t = base.clone()                                         # all keys equal: every weight 1 / S, the output the mean of v
    t[:, 1] = t[0, 1]
    out.append(("ties", t))
    sign = 1.0 - 2.0 * (torch.arange(dh, dtype=torch.float64) % 2)
    for nm, a, tt in (("offset1e3", 1.0, 200.0), ("offset1e4", 7.0, 41.0)):
        # u added to every query, t u to every key: every score gains t |u|^2 / sqrt(dh) (980 / 9840 at dh = 24) + a per-query constant
        u = a * sign
        t = base.clone()
        t[:, 0] += u
        t[:, 1] += tt * u
        out.append((nm, t))
    for p in dominant_positions(S):
        t = base.clone().view(nseq, S, 3, heads, dh)
        t[:, p, 1] = 25.0 * t[:, 3 % S, 0]                   # key p aligned with query 3 (mod S): one weight ~1 there, a spread of weights elsewhere
        out.append(("dominant%d" % p, t.view(nseq * S, 3, heads, dh)))
    t = base.clone()                                         # every score near -24 * 64 / sqrt(dh) = -313
    t[:, 0] += 8.0
    t[:, 1] -= 8.0
    out.append(("negative", t))
    return [(nm, t.reshape(nseq * S, 3 * D).to(dtype)) for nm, t in out]


def softmax_bar(qkv, heads, base_tol):
    """the op's own tolerance + 2 max|v| ds, ds = dh 2^-24 max|q| max|k| / sqrt(dh): an fp32-rounded score moves a softmax weight by that relative amount"""
    D = qkv.shape[1] // 3
    dh = D // heads
    q, k, v = (qkv[:, i * D:(i + 1) * D].double().abs().max().item() for i in range(3))
    return base_tol + 2.0 * v * dh * 2.0 ** -24 * q * k / math.sqrt(dh)
