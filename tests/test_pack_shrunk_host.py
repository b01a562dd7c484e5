"""packing.pack_vit_shrunk against cfen_oracle.vit_tokens, in float64 on the CPU: the packed matrices applied to zero-padded tokens -- LayerNorm over
the real slots, softmax at 1 / sqrt(dh_pad) on the padded heads, as csrc/cfen_net.cpp runs the v5 LViT blocks -- equal the oracle on the real
tokens, and every padding slot of every intermediate is an exact zero.  That pins the scatter maps of the residual-stream and attention axes, the
sqrt(dh_pad / dh) on W_q, and the zero rows of gamma / beta / bias the kernels rely on.  test_hip_ops.test_v5_block_on_the_padded_layout runs
the same block from the operators on the device, on geometry() and block_weights() of this module."""
import math

import pytest
import torch

import cfen_oracle
from cfen_vit_dehazing_amd import packing
from cfen_vit_dehazing_amd.config import NetConfig

# (C, cs, heads) of the v5 LViT levels at n_feats 24; p = 2, windows of 8 x 8 pixels = 16 tokens
GEOMETRIES = [(6, 8, 4), (12, 16, 8), (24, 24, 16)]
WS, NWIN = 8, 3


def geometry(C):
    cfg = NetConfig(24, 4, patch_size=WS, load_size=8 * WS, variant="v5")
    g = cfg.vit("localvit_encoder_0%d" % {6: 1, 12: 2, 24: 3}[C])
    assert (g.channels, g.patch, g.seq, g.dim, g.hidden, g.shrink) == (C, 2, 16, 4 * C, 16 * C, 4)
    return g


def block_weights(g, seed=0, dtype=torch.float64):
    """a seeded state dict of one block (the entries cfen_oracle.vit_tokens reads), every LayerNorm / bias vector nonzero everywhere"""
    gen = torch.Generator().manual_seed(300 + seed)
    D, H, n, e = g.dim, g.hidden, g.name, g.name + ".encoder.layers.0"
    rn = lambda *shape, s=1.0: (s * torch.randn(*shape, generator=gen, dtype=torch.float64)).to(dtype)
    sd = {n + ".linear_encoding.weight": rn(D, D, s=D ** -0.5), n + ".linear_encoding.bias": rn(D, s=0.1) + 0.3,
          n + ".position_encoding.pe.weight": rn(g.seq, D), e + ".self_attn.in_proj_weight": rn(3 * D, D, s=D ** -0.5),
          e + ".self_attn.out_proj.weight": rn(D, D, s=D ** -0.5),
          e + ".linear1.weight": rn(H, D, s=D ** -0.5), e + ".linear1.bias": rn(H, s=0.1) + 0.3,
          e + ".linear2.weight": rn(D, H, s=H ** -0.5), e + ".linear2.bias": rn(D, s=0.1) + 0.3,
          n + ".mlp_head.0.weight": rn(H, D, s=D ** -0.5), n + ".mlp_head.0.bias": rn(H, s=0.1) + 0.3,
          n + ".mlp_head.3.weight": rn(D, H, s=H ** -0.5), n + ".mlp_head.3.bias": rn(D, s=0.1) + 0.3}
    for k in ("norm1", "norm2"):
        sd["%s.%s.weight" % (e, k)], sd["%s.%s.bias" % (e, k)] = 1 + rn(D, s=0.1), rn(D, s=0.1) + 0.3
    return sd


def token_slots(g, cs):
    """slot of oracle feature f = c * p * p + ij in the padded token row: ij * cs + c"""
    f = torch.arange(g.dim)
    return (f % (g.patch ** 2)) * cs + f // (g.patch ** 2)


def padded_block(pk, g, cs, tokp, taps=None):
    """the block of csrc/cfen_net.cpp's unfused route in torch, in tokp's precision, on padded tokens (M, p * p * cs) with the packed entries `pk`;
    taps[name] = the intermediates whose padding slots must be zero"""
    n = g.name
    W = lambda k: pk[n + k].to(tokp.dtype)
    heads, dhp = g.heads, packing.round_up(g.dim // g.heads, 8)
    Da = heads * dhp
    real = torch.zeros(g.patch ** 2 * cs, dtype=torch.bool)
    real[token_slots(g, cs)] = True
    keep = (lambda k, t: taps.__setitem__(k, t)) if taps is not None else (lambda k, t: None)

    def ln(x, k):
        out = W(k + ".b").expand(x.shape).clone()            # a padding slot comes out as beta (include/cfen_padnorm.h), which the packer made 0
        out[:, real] = cfen_oracle.layer_norm(x[:, real], W(k + ".g")[real], W(k + ".b")[real])
        return out
    M = tokp.shape[0]
    x = tokp @ W(".embed.w").t() + W(".embed.b") + tokp + W(".pos").repeat(M // g.seq, 1)
    keep("embed", x)
    qkv = ln(x, ".ln1") @ W(".qkv.w").t()
    q, k, v = (t.reshape(M // g.seq, g.seq, heads, dhp).transpose(1, 2) for t in qkv.split(Da, dim=-1))
    a = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(dhp), dim=-1) @ v).transpose(1, 2).reshape(M, Da)
    keep("attention", a)
    x = x + a @ W(".proj.w").t()
    keep("proj", x)
    h = torch.relu(ln(x, ".ln2") @ W(".ffn1.w").t() + W(".ffn1.b"))
    x = x + h @ W(".ffn2.w").t() + W(".ffn2.b")
    keep("ffn2", x)
    h = torch.relu(x @ W(".head1.w").t() + W(".head1.b"))
    x = x + h @ W(".head2.w").t() + W(".head2.b")
    keep("head2", x)
    return x


@pytest.mark.parametrize("C,cs,heads", GEOMETRIES)
def test_pack_vit_shrunk_is_the_oracle_block_on_padded_tokens(C, cs, heads):
    g = geometry(C)
    assert g.heads == heads and packing.cs_of(C) == cs
    sd = block_weights(g)
    gen = torch.Generator().manual_seed(7 + C)
    tok = torch.randn(NWIN, g.seq, g.dim, generator=gen, dtype=torch.float64)
    want = cfen_oracle.vit_tokens(sd, g.name, tok, heads)
    pk = packing.pack_vit_shrunk(sd, g, torch.float64)
    slots = token_slots(g, cs)
    Dp = g.patch ** 2 * cs
    tokp = torch.zeros(NWIN * g.seq, Dp, dtype=torch.float64)
    tokp[:, slots] = tok.reshape(-1, g.dim)
    taps = {}
    got = padded_block(pk, g, cs, tokp, taps)
    err = float((got[:, slots] - want.reshape(-1, g.dim)).abs().max())
    print("(C %d, cs %d, heads %d): max-abs distance from vit_tokens %.3e at max |want| %.3g" % (C, cs, heads, err, float(want.abs().max())))
    # rounding of float64: a few hundred operations per output on values of order 1 .. 10
    assert err <= 1e-12 * max(1.0, float(want.abs().max()))
    pad = torch.ones(Dp, dtype=torch.bool)
    pad[slots] = False
    assert int(pad.sum()) == Dp - g.dim
    for name in ("embed", "proj", "ffn2", "head2"):
        assert bool((taps[name][:, pad] == 0).all()), "%s: a padding slot is not an exact zero" % name
    # the padded head dims of q, k, v and of the attention output are exact zeros too
    dh, dhp = g.dim // heads, packing.round_up(g.dim // heads, 8)
    hpad = torch.arange(heads * dhp) % dhp >= dh
    assert bool((taps["attention"][:, hpad] == 0).all()) and int(hpad.sum()) == heads * (dhp - dh)
    # gamma, beta and the residual-stream biases are zero in the padding slots, nonzero in the real ones
    for k in (".ln1.g", ".ln1.b", ".ln2.g", ".ln2.b", ".embed.b", ".ffn2.b", ".head2.b"):
        assert bool((pk[g.name + k][pad] == 0).all()) and bool((pk[g.name + k][~pad] != 0).all()), k
    # W_q carries sqrt(dh_pad / dh), W_k and W_v do not
    w_in = sd[g.name + ".encoder.layers.0.self_attn.in_proj_weight"]
    apos = (torch.arange(g.dim) // dh) * dhp + torch.arange(g.dim) % dh
    for t, f in enumerate((math.sqrt(dhp / dh), 1.0, 1.0)):
        assert torch.equal(pk[g.name + ".qkv.w"][t * heads * dhp + apos][:, slots], w_in[t * g.dim:(t + 1) * g.dim] * f)


def test_float32_packing_is_what_it_was():
    """the float64 route above changes nothing for the dtypes the kernels take: the vectors stay float32, the matrices are the float32-scattered ones"""
    g = geometry(6)
    sd = block_weights(g, dtype=torch.float32)
    pk = packing.pack_vit_shrunk(sd, g, torch.float16)
    assert pk[g.name + ".ln1.g"].dtype == torch.float32 and pk[g.name + ".qkv.w"].dtype == torch.float16
    w_in = sd[g.name + ".encoder.layers.0.self_attn.in_proj_weight"]
    apos, slots = (torch.arange(24) // 6) * 8 + torch.arange(24) % 6, token_slots(g, 8)
    assert torch.equal(pk[g.name + ".qkv.w"][apos][:, slots], (w_in[:24] * math.sqrt(8 / 6)).to(torch.float16))
