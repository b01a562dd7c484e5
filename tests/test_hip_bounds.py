"""Every kernel-launching entry point of include/cfen_hip.h once between guard bands (tests/guarded.py).

Each call gets every input in a guarded tensor whose bands are 0xff bytes (NaN to a float kernel that reads past an end, 255 to a byte kernel)
and every output and scratch buffer in a guarded tensor prefilled with 0xff bytes between random bands.  Asserted, in this order: no band
changed; every element the operator's contract says it writes matches the float64 / oracle reference at the bar of the operator's own test
(tests/test_hip_ops.py and its neighbours: `close`, `tol`, `rnd` are theirs, no new tolerance) -- an element that was never written is still NaN
and fails there; the padding lanes of an NHWC output hold what the contract in include/cfen_hip.h says (exact zeros, or the prefill untouched);
byte outputs are the same bytes on a zero-prefilled output and nothing outside the written region changed; scratch keeps its post-condition.

Shapes are the smallest ragged ones of the operators' own tests.  COVERED / NOT_COVERED list the header's entry points; tests/test_cabi.py checks
without a GPU that the two cover every function of the header that launches a kernel.

What this cannot see: a stray access further out than a band (64 KiB, or one row of the tensor if that is more), and an over-read whose value
never reaches a result -- NaN bands catch only the over-reads that do."""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cfen_oracle
import dcn_ref
from cfen_vit_dehazing_amd import _lib, ops, packing
from cfen_vit_dehazing_amd._lib import check, current_stream, ptr
from guarded import check_bands, guarded_copy, guarded_empty, raw_bytes, refill
from helpers import GOLDEN
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from test_hip_dcn import HW_GEOMETRIES, _grads_close, _out_close, _problem, _ref_backward
from test_hip_ops import DTYPES, _chain_ref, _lvit_instance, attn_ref, close, dev, perm_tokens, rnd, to_head_major, tol

pytestmark = pytest.mark.gpu

# entry point of include/cfen_hip.h -> the test below that runs it between bands
COVERED = {
    "cfen_gemm_nt": "test_gemm_nt", "cfen_gemm_ln": "test_gemm_ln", "cfen_gemm_splitk": "test_gemm_splitk", "cfen_gemm_chain": "test_gemm_chain",
    "cfen_embed_gather": "test_embed_gather", "cfen_embed_qkv": "test_embed_qkv", "cfen_embed_qkv_stream": "test_embed_qkv_stream",
    "cfen_layernorm": "test_layernorm", "cfen_attention": "test_attention", "cfen_attention_head_major": "test_attention_head_major",
    "cfen_mlp_block": "test_mlp_block", "cfen_mlp_stream_block": "test_mlp_stream_block", "cfen_lvit_window": "test_lvit_window",
    "cfen_patchify": "test_patchify_unpatchify", "cfen_unpatchify": "test_patchify_unpatchify", "cfen_upsample4": "test_upsample4",
    "cfen_nchw_to_nhwc": "test_input_layout_kernels", "cfen_u8hwc_to_nhwc": "test_input_layout_kernels", "cfen_tensor2im_u8": "test_tensor2im_u8",
    "cfen_conv2d": "test_conv_gather", "cfen_head_conv5": "test_head_conv5", "cfen_instnorm_relu": "test_instnorm_relu", "cfen_cfsm2g": "test_cfsm2g",
    "cfen_tile_gather": "test_tile_gather", "cfen_tile_blend": "test_tile_blend", "cfen_x8_expand": "test_x8_expand_and_merge",
    "cfen_x8_merge": "test_x8_expand_and_merge", "cfen_image_metrics": "test_image_metrics", "cfen_image_msssim": "test_image_msssim",
    "cfen_png_deflate": "test_png_deflate",
    "cfen_deform_conv_forward": "test_deform_conv_forward", "cfen_deform_conv_forward_nhwc": "test_deform_conv_forward_nhwc",
    "cfen_modulated_deform_conv_forward_nhwc": "test_deform_conv_forward_nhwc", "cfen_deform_conv_backward_input": "test_deform_conv_backward",
    "cfen_deform_conv_backward_parameters": "test_deform_conv_backward",
    "cfen_modulated_deform_conv_forward": "test_modulated_deform_conv", "cfen_modulated_deform_conv_backward": "test_modulated_deform_conv",
}
_NET = "whole generator: tests/test_hip_net_memory.py runs it on a guarded workspace, output slab and input"
NOT_COVERED = {
    "cfen_net_forward": _NET, "cfen_net_graph_capture": _NET, "cfen_net_graph_launch": _NET,
    "cfen_net_profile": "the forward's launches between HIP events: the same kernels on the same workspace as cfen_net_forward",
}


def G(t, name=None):
    """an input: the operand's values on the device between NaN bands"""
    return guarded_copy(t, device=dev(), name=name)


def O(shape, dtype, name=None, fill="ff"):
    """an output or scratch buffer on the device, prefilled, between random bands"""
    return guarded_empty(shape, dtype, dev(), fill, name=name)


def bands(*ts):
    torch.cuda.synchronize()
    check_bands(*[t for t in ts if t is not None])


def padding_zero(out, C, what):
    assert out.shape[-1] > C, "%s: no padding lanes at this shape" % what
    assert float(out[..., C:].float().abs().max()) == 0.0, "%s: padding lanes are not exact zeros" % what


def padding_untouched(out, C, what):
    """the contract 'padding left untouched': the lanes past C still hold the 0xff prefill, bit for bit"""
    assert out.shape[-1] > C, "%s: no padding lanes at this shape" % what
    lanes = out[..., C:].contiguous().view(torch.uint8)
    assert bool((lanes == 255).all()), "%s: padding lanes were written (the contract says they are left untouched)" % what


def nhwc(x, cs=None):
    return ops.to_nhwc(x, cs=cs)


# ---- GEMM family ------------------------------------------------------------------------------------------------------------------------------
def ksteps(dtype, n):
    return n * (32 if dtype == torch.float32 else 64)


def _gemm_operands(dtype, M, N, K):
    x, w = rnd((M, K), 1, dtype), rnd((N, K), 2, dtype, 1 / math.sqrt(K))
    bias, res, pos = rnd((N,), 3, torch.float32), rnd((M, N), 4, dtype), rnd((16, N), 5, dtype)
    ref = x.double() @ w.double().t()
    full = torch.relu(ref + bias.double()) + res.double() + pos.double()[torch.arange(M) % 16]
    return x, w, bias, res, pos, ref, full


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,ks,knobs", [(37, 48, None, {}), (257, 100, 17, {}), (1, 4, 1, {}), (130, 776, None, {"gemm.kernel": 6})],
                         ids=["37x48x64", "257x100x17steps", "1x4x1step", "big_tile_130x776x128"])
def test_gemm_nt(dtype, M, N, ks, knobs):
    K = ksteps(dtype, ks) if ks else (64 if M == 37 else 128)
    x, w, bias, res, pos, ref, full = _gemm_operands(dtype, M, N, K)
    gx, gw, gb, gr, gp = G(x, "x"), G(w, "w"), G(bias, "bias"), G(res, "residual"), G(pos, "pos")
    y, y2 = O((M, N), dtype, "y plain"), O((M, N), dtype, "y epilogue")
    with ops.tuning(knobs):
        ops.gemm_nt(gx, gw, out=y)
        ops.gemm_nt(gx, gw, bias=gb, residual=gr, pos=gp, relu=True, out=y2)
    bands(gx, gw, gb, gr, gp, y, y2)
    close(y, ref, tol(dtype, 4), "plain")
    close(y2, full, tol(dtype, 8), "bias+relu+res+pos")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_ln(dtype):
    M, D, N = 7, 3072, 96
    x = rnd((M, D), 1, dtype, 2.0) + 1.0
    w = rnd((N, D), 2, torch.float32, D ** -0.5)
    g, b, bias = 1 + 0.1 * rnd((D,), 3, torch.float32), 0.1 * rnd((D,), 4, torch.float32), rnd((N,), 5, torch.float32)
    want = (cfen_oracle.layer_norm(x.double(), g.double(), b.double()) @ w.double().t() + bias.double()).relu()
    f = packing.ln_folded(None, g, b, bias, "l", dtype, w)
    ins = [G(x, "x"), G(f["l.wl"], "wl"), G(f["l.s"], "s"), G(f["l.bl"], "bias")]
    y = O((M, N), dtype, "y")
    ops.gemm_ln(*ins, relu=True, out=y)
    bands(y, *ins)
    close(y, want, tol(dtype, 8))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,nsplit", [(33, 96, 256, 2), (100, 200, 768, 2)])
def test_gemm_splitk(dtype, M, N, K, nsplit):
    """the scratch starts zeroed, as its contract requires (only its bands are patterned); its arrival counters are zero again after the call"""
    x, w, bias, res, _, ref, _ = _gemm_operands(dtype, M, N, K)
    tiles = ((N + 95) // 96) * ((M + 31) // 32)
    scratch = O((4096 + tiles * nsplit * 14336,), torch.uint8, "split-K scratch", fill="zero")
    gx, gw, gb, gr = G(x, "x"), G(w, "w"), G(bias, "bias"), G(res, "residual")
    y, y2 = O((M, N), dtype, "y plain"), O((M, N), dtype, "y epilogue")
    ops.gemm_splitk(gx, gw, nsplit, scratch=scratch, out=y)
    ops.gemm_splitk(gx, gw, nsplit, bias=gb, residual=gr, relu=True, scratch=scratch, out=y2)
    bands(gx, gw, gb, gr, y, y2, scratch)
    close(y, ref, tol(dtype, 4), "plain")
    close(y2, torch.relu(ref + bias.double()) + res.double(), tol(dtype, 6), "bias + relu + residual")
    assert int(scratch[:4096].view(torch.int32).abs().sum()) == 0, "arrival counters are not back to zero"


def test_gemm_chain():
    """the smallest shape of test_gemm_chain_single_phase; the sync buffer is prefilled 0xff (the call zeroes the words it needs) and its error word ends zero"""
    M, N, K, nsplit, team = 16, 128, 64, 1, 3
    dt = torch.float16
    x, w, bias, res, pos, _, _ = _gemm_operands(dt, M, N, K)
    gx, gs, gb, gr, gp = G(x, "x"), G(packing.pack_stream_tiles(w.contiguous()), "w stream"), G(bias, "bias"), G(res, "residual"), G(pos, "pos")
    y = O((M, N), dt, "y")
    sync = O((8192 + ((M + 127) // 128) * (N // 128) * nsplit * 65536,), torch.uint8, "chain sync + slabs")
    ops.gemm_chain([dict(x=gx, w_stream=gs, N=N, K=K, y=y, bias=gb, residual=gr, pos=gp, relu=True, nsplit=nsplit)], M, team, sync=sync)
    bands(gx, gs, gb, gr, gp, y, sync)
    close(y, _chain_ref(x, w, bias, None, res, pos, True), tol(dt, 8), "bias + relu + residual + pos")
    assert int(sync[:8].view(torch.int32)[1]) == 0, "the chain's error word is set"


def _embed_operands(dtype, B, C, H, W, ws, p=2):
    D = p * p * C
    S = (ws // p) ** 2
    x = rnd((B, C, H, W), 1, dtype)
    we, be = rnd((D, D), 2, dtype, 1 / math.sqrt(D)), rnd((D,), 3, torch.float32, 0.1)
    pos = rnd((S, D), 4, dtype)
    g, b = 1 + rnd((D,), 5, torch.float32, 0.1), rnd((D,), 6, torch.float32, 0.1)
    wq = rnd((3 * D, D), 7, dtype, 1 / math.sqrt(D))
    tok = perm_tokens(cfen_oracle.unfold_tokens(cfen_oracle.window_partition(x.float(), ws), p), C, p).reshape(-1, D).double()
    y = tok @ we.double().t() + be.double() + tok + pos.double().repeat(tok.shape[0] // S, 1)
    qkv = F.layer_norm(y, (D,), g.double(), b.double(), 1e-5) @ wq.double().t()
    return x, we, be, pos, g, b, wq, y, qkv, D, S


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_gather(dtype):
    B, C, H, W, ws = 3, 24, 64, 32, 32
    x, we, be, pos, _, _, _, y, _, D, S = _embed_operands(dtype, B, C, H, W, ws)
    ins = [G(nhwc(x), "fmap"), G(we, "w"), G(be, "bias"), G(pos, "pos")]
    out = O((B * H * W // 4, D), dtype, "y")
    ops.embed_gather(ins[0], C, ws, 2, ins[1], ins[2], ins[3], out=out)
    bands(out, *ins)
    close(out, y, tol(dtype, 4))


@pytest.mark.parametrize("dtype", DTYPES)
def test_embed_qkv(dtype):
    B, C, H, W, ws = 3, 24, 64, 32, 32
    x, we, be, pos, g, b, wq, y, qkv, D, S = _embed_operands(dtype, B, C, H, W, ws)
    perm = packing.kperm32(D) if dtype == torch.float16 else torch.arange(D)
    ins = [G(nhwc(x), "fmap"), G(we[:, perm].contiguous(), "we"), G(be, "be"), G(pos, "pos"), G(g, "ln gamma"), G(b, "ln beta"), G(wq[:, perm].contiguous(), "wqkv")]
    M = B * H * W // 4
    x1, q = O((M, D), dtype, "x1"), O((M, 3 * D), dtype, "qkv")
    ops.embed_qkv(ins[0], C, ws, 2, *ins[1:], out=(x1, q))
    bands(x1, q, *ins)
    close(x1, y, tol(dtype, 4), "x1")
    close(q, qkv, tol(dtype, 6), "qkv")


def test_embed_qkv_stream():
    dtype = torch.float16
    B, C, H, W, ws, heads = 2, 96, 32, 64, 16, 16
    x, we, be, pos, g, b, wq, y, qkv, D, S = _embed_operands(dtype, B, C, H, W, ws)
    kd = packing.kperm32(D)
    ins = [G(nhwc(x), "fmap"), G(packing.pack_stream_rows(we[:, kd]), "we stream"), G(be, "be"), G(pos, "pos"), G(g, "ln gamma"), G(b, "ln beta"),
           G(packing.pack_stream_rows(wq[:, kd]), "wqkv stream")]
    M = B * H * W // 4
    x1, q = O((M, D), dtype, "x1"), O((M, 3 * D), dtype, "qkv")
    ops.embed_qkv(ins[0], C, ws, 2, *ins[1:], stream_weights=True, out=(x1, q))
    bands(x1, q, *ins)
    close(x1, y, tol(dtype, 6), "x1")
    close(q, qkv, tol(dtype, 12), "qkv")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", [(5, 96), (7, 2048), (2, 2048)])
def test_layernorm(dtype, M, D):
    x = rnd((M, D), 1, dtype, 2.0) + 0.5
    g, b = 1 + 0.1 * rnd((D,), 2, torch.float32), 0.1 * rnd((D,), 3, torch.float32)
    ins = [G(x, "x"), G(g, "gamma"), G(b, "beta")]
    y = O((M, D), dtype, "y")
    ops.layernorm(*ins, out=y)
    bands(y, *ins)
    close(y, cfen_oracle.layer_norm(x.double(), g.double(), b.double()), tol(dtype, 4))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,cs,C", [(5, 8, 6), (33, 16, 12)])
def test_guard_bands_padnorm(dtype, M, cs, C):
    """include/cfen_padnorm.h through the C ABI: rows of 4 pixels of cs slots, C of them real, the padding slots of x NaN (they are never read into a
    result); the padding slots of y come out as beta = 0.  Then four refused calls: y keeps its prefill"""
    import padnorm_ref as pr
    lib = _lib.load()
    D, real = 4 * cs, pr.real_slots(cs, C)
    x = pr.scatter(rnd((M, 4 * C), 1, dtype, 2.0) + 0.5, cs, C, fill=float("nan"))
    g, b = pr.scatter(1 + 0.1 * rnd((4 * C,), 2, torch.float32), cs, C), pr.scatter(0.1 * rnd((4 * C,), 3, torch.float32), cs, C)
    ins = [G(x, "x"), G(g, "gamma"), G(b, "beta")]
    y = O((M, D), dtype, "y")
    call = lambda M_, D_, cs_, C_: lib.cfen_layernorm_padded(_lib.dtype_code(dtype), ptr(ins[0]), ptr(y), ptr(ins[1]), ptr(ins[2]), M_, D_, cs_, C_, 1e-5,
                                                             current_stream())
    for bad in ((M, D, cs, cs + 1), (M, D, cs, 0), (M, D + 8, 16, C), (0, D, cs, C)):
        assert call(*bad) == -1 and b"layernorm" in lib.cfen_last_error(), bad
    bands(y, *ins)
    assert bool((raw_bytes(y) == 255).all()), "a refused call wrote its output"
    check(call(M, D, cs, C), "layernorm_padded")
    bands(y, *ins)
    on = real.to(y.device)
    close(y[:, on], cfen_oracle.layer_norm(x[:, real].double(), g[real].double(), b[real].double()), tol(dtype, 4))
    assert bool((y[:, ~on] == 0).all()), "padding slots are not beta = 0"


# head dims 4 and 12 run in fp32 only (fragment width 4, not fp16's 8)
ATTENTION = [(dt,) + c for dt in DTYPES for c in ((2, 1, 16, 24), (2, 4, 8, 24), (3, 256, 4, 24), (2, 16, 4, 8), (2, 80, 1, 128))] + \
            [(torch.float32, 3, 16, 4, 4), (torch.float32, 2, 64, 8, 12)]


@pytest.mark.parametrize("dtype,nseq,S,heads,dh", ATTENTION)
def test_attention(dtype, nseq, S, heads, dh):
    qkv = rnd((nseq * S, 3 * heads * dh), 7, dtype, 1.5)
    gq = G(qkv, "qkv")
    out = O((nseq * S, heads * dh), dtype, "out")
    ops.attention(gq, nseq, S, heads, out=out)
    bands(gq, out)
    close(out, attn_ref(qkv, nseq, S, heads), tol(dtype, 3))


@pytest.mark.parametrize("nseq,S,heads,pair", [(2, 64, 4, 0), (3, 256, 4, 0), (3, 256, 4, 1)])
def test_attention_head_major(nseq, S, heads, pair):
    """(2, 64, 4), and S = 256 on k_attention_hm and on the long-window kernel ("attn.hm_pair" 1: another store pattern)"""
    qkv = rnd((nseq * S, 3 * heads * 24), 7, torch.float16, 1.5)
    gq = G(to_head_major(qkv, nseq, S, heads), "qkv head-major")
    out = O((nseq * S, heads * 24), torch.float16, "out")
    with ops.tuning({"attn.hm_pair": pair}):
        ops.attention_head_major(gq, nseq, S, heads, out=out)
    bands(gq, out)
    close(out, attn_ref(qkv, nseq, S, heads), tol(torch.float16, 3))


# ---- fused token blocks ---------------------------------------------------------------------------------------------------------------------------
def _mlp_operands(dtype, D, H, M):
    x = rnd((M, D), 1, dtype)
    g, b = 1 + 0.1 * rnd((D,), 2, torch.float32), 0.1 * rnd((D,), 3, torch.float32)
    w1a, w2a = rnd((H, D), 4, dtype, D ** -0.5), rnd((D, H), 5, dtype, 0.5 * H ** -0.5)
    w1b, w2b = rnd((H, D), 6, dtype, D ** -0.5), rnd((D, H), 7, dtype, 0.5 * H ** -0.5)
    b1a, b2a, b1b, b2b = (0.1 * rnd((n,), 8 + i, torch.float32) for i, n in enumerate((H, D, H, D)))
    xd = x.double()
    y1 = xd + torch.relu(cfen_oracle.layer_norm(xd, g.double(), b.double()) @ w1a.double().t() + b1a.double()) @ w2a.double().t() + b2a.double()
    y2 = y1 + torch.relu(y1 @ w1b.double().t() + b1b.double()) @ w2b.double().t() + b2b.double()
    return x, g, b, (w1a, w2a), (w1b, w2b), (b1a, b2a, b1b, b2b), y2


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,H,M", [(96, 192, 64), (192, 384, 130)])
def test_mlp_block(dtype, D, H, M):
    x, g, b, wa, wb, (b1a, b2a, b1b, b2b), y2 = _mlp_operands(dtype, D, H, M)
    if dtype == torch.float16:
        kd, kh = packing.kperm32(D), packing.kperm32(H)
        wa, wb = (wa[0][:, kd].contiguous(), wa[1][:, kh].contiguous()), (wb[0][:, kd].contiguous(), wb[1][:, kh].contiguous())
    ins = [G(x, "x"), G(wa[0], "w1a"), G(b1a, "b1a"), G(wa[1], "w2a"), G(b2a, "b2a")]
    ln, second = (G(g, "ln gamma"), G(b, "ln beta")), (G(wb[0], "w1b"), G(b1b, "b1b"), G(wb[1], "w2b"), G(b2b, "b2b"))
    y = O((M, D), dtype, "y")
    ops.mlp_block(*ins, ln=ln, second=second, out=y)
    bands(y, *ins, *ln, *second)
    close(y, y2, tol(dtype, 10), "both stages")


def host_unpatchify(tok, B, C, H, W, ws, p):
    """the (B, C, H, W) float64 map whose tokens are `tok`, on the host, by the oracle's own token gather run on element indices: no kernel under test
    takes part in a fold test's reference"""
    n = B * C * H * W
    idx = torch.arange(n, dtype=torch.float64).view(B, C, H, W)
    where = perm_tokens(cfen_oracle.unfold_tokens(cfen_oracle.window_partition(idx, ws), p), C, p).reshape(-1).long()
    assert where.numel() == n == tok.numel() and torch.equal(where.sort().values, torch.arange(n))
    out = torch.empty(n, dtype=torch.float64)
    out[where] = tok.reshape(-1).double()
    return out.view(B, C, H, W)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,H,C,cs", [(96, 192, 24, 32), (192, 384, 48, 56)])
def test_mlp_block_fold(dtype, D, H, C, cs):
    """fold= into an NHWC map with cs > C (test_fused_mlp_fold_epilogue's geometry, and the D 192 kernel on 48 channels in a stride of 56): the raw map
    holds the float64 result unpatchified on the host; the contract for the padding lanes is 'left untouched' (include/cfen_hip.h), like cfen_unpatchify's"""
    B, Hm, Wm, ws, pp = 2, 16, 32, 8, 2
    M = B * Hm * Wm // 4
    x = rnd((M, D), 1, dtype)
    w1, w2 = rnd((H, D), 2, dtype, D ** -0.5), rnd((D, H), 3, dtype, H ** -0.5)
    b1, b2 = 0.1 * rnd((H,), 4, torch.float32), 0.1 * rnd((D,), 5, torch.float32)
    want = x.double() + torch.relu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
    if dtype == torch.float16:
        w1, w2 = w1[:, packing.kperm32(D)].contiguous(), w2[:, packing.kperm32(H)].contiguous()
    ins = [G(x, "x"), G(w1, "w1"), G(b1, "b1"), G(w2, "w2"), G(b2, "b2")]
    fm = O((B, Hm, Wm, cs), dtype, "folded map")
    ops.mlp_block(*ins, fold=(B, Hm, Wm, C, cs, ws, pp), out=fm)
    bands(fm, *ins)
    close(ops.from_nhwc(fm, C), host_unpatchify(want, B, C, Hm, Wm, ws, pp), tol(dtype, 6), "folded values")
    padding_untouched(fm, C, "mlp_block(fold=)")


@pytest.mark.parametrize("D,H,M,pair", [(384, 96, 31, 1), (192, 384, 256, 1), (384, 256, 130, 1), (384, 256, 130, 0)],
                         ids=["384x96x31", "192x384x256", "pair_kernel_256x130", "single_kernel_256x130"])
def test_mlp_stream_block(D, H, M, pair):
    dtype = torch.float16
    x, g, b, wa, wb, (b1a, b2a, b1b, b2b), y2 = _mlp_operands(dtype, D, H, M)
    kd, kh = packing.kperm32(D), packing.kperm32(H)
    sa, sb = G(packing.pack_stream_pair(wa[0][:, kd], wa[1][:, kh]), "wa stream"), G(packing.pack_stream_pair(wb[0][:, kd], wb[1][:, kh]), "wb stream")
    ins = [G(x, "x"), sa, G(b1a, "b1a"), G(b2a, "b2a"), G(g, "ln gamma"), G(b, "ln beta"), sb, G(b1b, "b1b"), G(b2b, "b2b")]
    y = O((M, D), dtype, "y")
    with ops.tuning({"mlp3.pair": pair}):
        ops.mlp_stream_block(ins[0], ins[1], ins[2], ins[3], H, ln=(ins[4], ins[5]), second=(ins[6], ins[7], ins[8]), out=y)
    bands(y, *ins)
    close(y, y2, tol(dtype, 10), "both stages")


def test_mlp_stream_block_fold():
    dtype = torch.float16
    B, C, Hm, Wm, ws, pp, cs = 2, 96, 16, 32, 8, 2, 104
    D, H = 384, 256
    M = B * Hm * Wm // 4
    x = rnd((M, D), 1, dtype)
    w1, w2 = rnd((H, D), 2, dtype, D ** -0.5), rnd((D, H), 3, dtype, H ** -0.5)
    b1, b2 = 0.1 * rnd((H,), 4, torch.float32), 0.1 * rnd((D,), 5, torch.float32)
    want = x.double() + torch.relu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double()
    ins = [G(x, "x"), G(packing.pack_stream_pair(w1[:, packing.kperm32(D)], w2[:, packing.kperm32(H)]), "w stream"), G(b1, "b1"), G(b2, "b2")]
    fm = O((B, Hm, Wm, cs), dtype, "folded map")
    ops.mlp_stream_block(*ins, H, fold=(B, Hm, Wm, C, cs, ws, pp), out=fm)
    bands(fm, *ins)
    close(ops.from_nhwc(fm, C), host_unpatchify(want, B, C, Hm, Wm, ws, pp), tol(dtype, 6), "folded values")
    padding_untouched(fm, C, "mlp_stream_block(fold=)")


def test_lvit_window():
    B, H, W = 1, 32, 32
    cfg, g, sd = _lvit_instance(3)
    dt = torch.float16
    sd16 = {k: (v.to(dt) if v.dtype.is_floating_point else v) for k, v in sd.items()}
    x = rnd((B, 24, H, W), 5, dt)
    want = cfen_oracle.lvit({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd16.items()}, g.name, x.double(), g.heads, 32)
    pk = packing.pack_vit(sd16, g, dt)
    pk.update(packing.pack_lvit_window(sd16, g, dt))
    pk = {k: G(v.contiguous(), k) for k, v in pk.items() if k.startswith(g.name)}
    fmap = G(nhwc(x), "fmap")
    out = O((B, H, W, 32), dt, "out map")                  # cs_out 32 > C 24
    ops.lvit_window(fmap, 24, 32, 2, pk, g.name, g.hidden, cs_out=32, out=out)
    bands(fmap, out, *pk.values())
    close(ops.from_nhwc(out, 24), want, tol(dt, 12), "fused window block vs fp64")
    padding_untouched(out, 24, "lvit_window")


# ---- token and layout kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_patchify_unpatchify(dtype):
    B, C, H, ws = 2, 24, 64, 16
    x = rnd((B, C, H, H), 1, dtype)
    fmap = G(nhwc(x, cs=32), "fmap")                      # cs > C on the input
    want = perm_tokens(cfen_oracle.unfold_tokens(cfen_oracle.window_partition(x.float(), ws), 2), C, 2).reshape(-1, 4 * C)
    tok = O(want.shape, dtype, "tokens")
    ops.patchify(fmap, C, ws, 2, out=tok)
    bands(fmap, tok)
    assert torch.equal(tok.float().cpu(), want)
    pooled = cfen_oracle.avgpool2(cfen_oracle.avgpool2(x.double()))
    want4 = perm_tokens(cfen_oracle.unfold_tokens(pooled, 4), C, 4).reshape(-1, 16 * C)
    tok4 = O(want4.shape, dtype, "pooled tokens")
    ops.patchify(fmap, C, H // 4, 4, pool=4, out=tok4)
    bands(fmap, tok4)
    close(tok4, want4, tol(dtype))
    # back into a map with cs 32 > C 24: every channel of every pixel is written, the padding lanes are left untouched (include/cfen_hip.h)
    gt = G(tok, "tokens in")
    back = O((B, H, H, 32), dtype, "map")
    ops.unpatchify(gt, B, H, H, C, 32, ws, 2, out=back)
    bands(gt, back)
    assert torch.equal(back[..., :C].cpu(), fmap[..., :C].cpu())
    padding_untouched(back, C, "unpatchify")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs_out", [8, 16])
def test_upsample4(dtype, cs_out):
    B, C, h, w = 2, 8, 5, 7
    x = rnd((B, C, h, w), 3, dtype)
    want = cfen_oracle.upsample2_bilinear(cfen_oracle.upsample2_bilinear(x.double()))
    small = G(nhwc(x), "small map")
    out = O((B, 4 * h, 4 * w, cs_out), dtype, "out map")
    ops.upsample4(small, cs_out=cs_out, out=out)
    bands(small, out)
    close(ops.from_nhwc(out, C), want, tol(dtype))
    if cs_out > C:
        padding_untouched(out, C, "upsample4")


@pytest.mark.parametrize("dtype", DTYPES)
def test_input_layout_kernels(dtype):
    """cs 8 with C 3: both kernels write the padding lanes themselves, as exact zeros"""
    x = rnd((2, 3, 16, 32), 4, torch.float32)
    gx = G(x, "x NCHW")
    out = O((2, 16, 32, 8), dtype, "NHWC")
    ops.nchw_to_nhwc(gx, 8, dtype, out=out)
    bands(gx, out)
    assert torch.equal(out.cpu(), ops.to_nhwc(x, cs=8).to(dtype))
    padding_zero(out, 3, "nchw_to_nhwc")
    img = torch.randint(0, 256, (2, 24, 40, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    gi = G(img, "image")
    out = O((2, 24, 40, 8), dtype, "NHWC")
    ops.u8hwc_to_nhwc(gi, 8, dtype, out=out)
    bands(gi, out)
    want = ((img.permute(0, 3, 1, 2).float() / 255.0) - 0.5) / 0.5
    assert torch.equal(out[..., :3].cpu(), want.permute(0, 2, 3, 1).to(dtype))
    padding_zero(out, 3, "u8hwc_to_nhwc")


def byte_outputs_agree(call, outs, written=None):
    """`call()` writes into `outs` (guarded, prefilled 0xff); run it, then again on a zero prefill: the written region (all of it, or `written(out)`: a
    bool mask over its bytes) is the same bytes, and every byte outside it still holds its prefill both times"""
    call()
    bands(*outs)
    first = [raw_bytes(o).clone() for o in outs]
    masks = [written(o) if written else None for o in outs]
    for o in outs:
        refill(o, "zero")
    call()
    bands(*outs)
    for o, a, m in zip(outs, first, masks):
        b = raw_bytes(o)
        if m is None:
            assert torch.equal(a, b), "the bytes depend on the output's prefill"
        else:
            m2 = written(o)
            assert torch.equal(m, m2) and torch.equal(a[m], b[m]), "the bytes depend on the output's prefill"
            assert bool((a[~m] == 255).all()) and bool((b[~m] == 0).all()), "bytes outside the written region were changed"
    return first


@pytest.mark.parametrize("C,H,W", [(3, 37, 53), (1, 5, 7)])
def test_tensor2im_u8(C, H, W):
    from cfen_vit_dehazing_amd.util import util
    x = torch.rand(C, H, W, generator=torch.Generator().manual_seed(H)) * 2 - 1
    gx = G(x, "x")
    out = O((H, W, 3), torch.uint8, "image")
    byte_outputs_agree(lambda: ops.tensor2im_u8(gx, out=out), [out])
    bands(gx)
    assert np.array_equal(out.cpu().numpy(), util.tensor2im(x))


# ---- convolutions ---------------------------------------------------------------------------------------------------------------------------------
def _conv_out(dtype, B, Hout, Wout, cout, nchw=False):
    if nchw:
        return O((B, cout, Hout, Wout), torch.float32, "out NCHW fp32")
    return O((B, Hout, Wout, packing.round_up(cout, 8)), dtype, "out map")


@pytest.mark.parametrize("wlds", [2, 0])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,k,stride,pad,size", [(3, 12, 5, 1, 2, 32), (12, 24, 3, 2, 1, 64), (4, 4, 3, 1, 1, 64)])
def test_conv_gather(dtype, cin, cout, k, stride, pad, size, wlds):
    """k_conv with the weights staged in LDS ("conv.wlds" 2) and read from global memory (0).  Padding lanes (12 in 16, 4 in 8): the kernel stores the whole
    channel stride, and the lanes past Cout are exact zeros because packing zero-fills their weight rows and affine entries"""
    kc = 32 if dtype == torch.float16 else 16
    x = rnd((2, cin, size, size), 1, dtype)
    w = rnd((cout, cin, k, k), 2, dtype, 1 / math.sqrt(cin * k * k))
    b = rnd((cout,), 3, torch.float32, 0.1)
    want = F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad)
    s, t = packing.affine(b, None, None, packing.round_up(cout, 16))
    ins = [G(nhwc(x), "x"), G(packing.pack_conv_weight(w, packing.cs_of(cin), kc, dtype)[0], "w"), G(s, "scale"), G(t, "shift")]
    out = _conv_out(dtype, 2, want.shape[2], want.shape[3], cout)
    with ops.tuning({"conv.wlds": wlds}):
        ops.conv2d(*ins, packing.cs_of(cin), cout, k=k, stride=stride, pad=pad, out=out)
    bands(out, *ins)
    close(ops.from_nhwc(out, cout), want, tol(dtype, 4))
    if out.shape[-1] > cout:
        padding_zero(out, cout, "conv2d (gather)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout,k,H,W", [(12, 12, 3, 8, 128), (12, 3, 7, 24, 192)])
def test_conv_rows_layout(dtype, cin, cout, k, H, W):
    x = rnd((2, cin, H, W), 1, dtype)
    w = rnd((cout, cin, k, k), 2, dtype, 1 / math.sqrt(cin * k * k))
    b, res = rnd((cout,), 3, torch.float32, 0.1), rnd((2, cout, H, W), 4, dtype)
    want = torch.relu(F.conv2d(x.double(), w.double(), b.double(), padding=k // 2)) + res.double()
    cs = packing.cs_of(cin)
    s, t = packing.affine(b, None, None, 16)
    ins = [G(nhwc(x), "x"), G(packing.pack_conv_weight_rows(w, cs, dtype)[0], "w rows"), G(s, "scale"), G(t, "shift")]
    gres = G(nhwc(res), "residual")
    out = _conv_out(dtype, 2, H, W, cout)
    ops.conv2d(*ins, cs, cout, k=k, stride=1, pad=k // 2, act=1, res0=gres, rows_layout=True, out=out)
    bands(out, gres, *ins)
    close(ops.from_nhwc(out, cout), want, tol(dtype, 4))
    padding_zero(out, cout, "conv2d (rows layout)")


@pytest.mark.parametrize("form", ["gather_fp32", "gather_fp16", "rows_fp16", "toeplitz_fp16"])
def test_conv_reflect7_tanh_nchw_fp32(form):
    dtype = torch.float32 if form.endswith("fp32") else torch.float16
    H, W = (32, 32) if form.startswith("gather") else (16, 64) if form.startswith("rows") else (32, 128)
    x = rnd((2, 12, H, W), 1, dtype)
    w = rnd((3, 12, 7, 7), 2, dtype, 0.3 / math.sqrt(12 * 49))
    b = rnd((3,), 3, torch.float32, 0.1)
    want = torch.tanh(F.conv2d(F.pad(x.double(), (3, 3, 3, 3), mode="reflect"), w.double(), b.double()))
    s, t = packing.affine(b, cout_pad=16)
    if form.startswith("gather"):
        wp, kw = packing.pack_conv_weight(w, 16, 32 if dtype == torch.float16 else 16, dtype)[0], {}
    elif form.startswith("rows"):
        wp, kw = packing.pack_conv_weight_rows(w, 16, dtype)[0], {"rows_layout": True}
    else:
        wp, kw = packing.pack_conv7_toeplitz(w, dtype)[0], {"toeplitz": True}
    ins = [G(nhwc(x), "x"), G(wp, "w"), G(s, "scale"), G(t, "shift")]
    out = _conv_out(dtype, 2, H, W, 3, nchw=True)
    ops.conv2d(*ins, 16, 3, k=7, stride=1, pad=3, reflect=True, act=2, nchw_f32=True, out=out, **kw)
    bands(out, *ins)
    close(out, want, tol(dtype, 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [24, 8])
def test_conv_1x1_concat_with_residual(dtype, C):
    kc = 32 if dtype == torch.float16 else 16
    a, b2 = rnd((2, C, 16, 16), 1, dtype), rnd((2, C, 16, 16), 2, dtype)
    w = rnd((C, 2 * C, 1, 1), 3, dtype, 1 / math.sqrt(2 * C))
    bias, anw, anb = rnd((C,), 4, torch.float32, 0.1), rnd((C,), 5, torch.float32, 0.2), rnd((C,), 6, torch.float32, 0.2)
    res = rnd((2, C, 16, 16), 7, dtype)
    y = F.conv2d(torch.cat((a, b2), 1).double(), w.double(), bias.double())
    want = torch.relu((y + anb.double().view(1, -1, 1, 1)) * torch.exp(anw.double()).view(1, -1, 1, 1)) + res.double()
    s, t = packing.affine(bias, anw, anb, packing.round_up(C, 16))
    ins = [G(nhwc(a), "src0"), G(packing.pack_conv_weight(w, packing.cs_of(C), kc, dtype)[0], "w"), G(s, "scale"), G(t, "shift")]
    g1, gr = G(nhwc(b2), "src1"), G(nhwc(res), "residual")
    out = _conv_out(dtype, 2, 16, 16, C)
    ops.conv2d(*ins, packing.cs_of(C), C, k=1, stride=1, pad=0, src1=g1, act=1, res0=gr, out=out)
    bands(out, g1, gr, *ins)
    close(ops.from_nhwc(out, C), want, tol(dtype, 6))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cin,cout", [(24, 12), (8, 4)])
def test_conv_transpose(dtype, cin, cout):
    kc = 32 if dtype == torch.float16 else 16
    x = rnd((2, cin, 16, 16), 1, dtype)
    w = rnd((cin, cout, 4, 4), 2, dtype, 1 / math.sqrt(cin * 4))
    b = rnd((cout,), 3, torch.float32, 0.1)
    want = torch.relu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    s, t = packing.affine(b, cout_pad=packing.round_up(cout, 16))
    ins = [G(nhwc(x), "x"), G(packing.pack_convT_weight(w, packing.cs_of(cin), kc, dtype), "w"), G(s, "scale"), G(t, "shift")]
    out = _conv_out(dtype, 2, 32, 32, cout)
    ops.conv2d(*ins, packing.cs_of(cin), cout, transpose=True, act=1, out=out)
    bands(out, *ins)
    close(ops.from_nhwc(out, cout), want, tol(dtype, 4))
    padding_zero(out, cout, "conv2d (transpose)")


def test_conv_transpose_rows_layout():
    dtype, cin, cout, H, W = torch.float16, 24, 12, 8, 32
    assert packing.convT_uses_rows_layout(dtype, packing.cs_of(cin), cout, H, W)
    x = rnd((2, cin, H, W), 1, dtype)
    w = rnd((cin, cout, 4, 4), 2, dtype, 1 / math.sqrt(cin * 4))
    b = rnd((cout,), 3, torch.float32, 0.1)
    want = torch.relu(F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1))
    s, t = packing.affine(b, cout_pad=16)
    ins = [G(nhwc(x), "x"), G(packing.pack_convT_weight_rows(w, packing.cs_of(cin), dtype), "w rows"), G(s, "scale"), G(t, "shift")]
    out = _conv_out(dtype, 2, 2 * H, 2 * W, cout)
    ops.conv2d(*ins, packing.cs_of(cin), cout, transpose=True, act=1, rows_layout=True, out=out)
    bands(out, *ins)
    close(ops.from_nhwc(out, cout), want, tol(dtype, 4))
    padding_zero(out, cout, "conv2d (transpose, rows layout)")


@pytest.mark.parametrize("u8", [False, True])
def test_head_conv5(u8):
    B, H, W = 1, 8, 64
    w, bias = rnd((12, 3, 5, 5), 1, torch.float16, 0.2), rnd((12,), 2, torch.float32)
    if u8:
        src = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
        x = ((src.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2)
    else:
        src = x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2 - 1
    gs = G(src.contiguous(), "network input")
    out = O((B, H, W, 16), torch.float16, "head map")
    ops.head_conv5(gs, w.to(dev()), bias.to(dev()), out=out)           # (the wrapper packs w / bias itself: they are not the caller's buffers)
    bands(gs, out)
    want = F.conv2d(x.half().double(), w.double(), bias.double(), padding=2).permute(0, 2, 3, 1)
    close(out[..., :12], want, tol(torch.float16, 4), "conv5 from the input")
    padding_zero(out, 12, "head_conv5")


def _stats(B):
    return O((_lib.load().cfen_stats_workspace(B, 128) // 4,), torch.float32, "stats workspace")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
def test_instnorm_relu(dtype, C):
    """in place: the bands of the map and the values; the stats workspace is prefilled 0xff and the result must not depend on that"""
    x = rnd((2, C, 16, 16), 1, dtype, 2.0) + 0.7
    want = torch.relu(cfen_oracle.instance_norm(x.double()))
    xn, ws = G(nhwc(x), "map (in place)"), _stats(2)
    ops.instnorm_relu_(xn, C, stats_ws=ws)
    bands(xn, ws)
    close(ops.from_nhwc(xn, C), want, tol(dtype, 2))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
def test_cfsm2g(dtype, C):
    h = C // 4
    g = torch.Generator().manual_seed(C)
    sd = {}
    for fc in ("fc_avg_cf1", "fc_avg_cf2", "fc_max_cf1", "fc_max_cf2"):
        sd["c.%s.0.weight" % fc] = torch.randn(h, C, 1, 1, generator=g) / math.sqrt(C)
        sd["c.%s.2.weight" % fc] = torch.randn(C, h, 1, 1, generator=g) / math.sqrt(h)
    xs = [rnd((2, C, 12, 20), 10 + i, dtype) for i in range(3)]
    w = torch.cat([sd["c.%s.%d.weight" % (fc, i)].reshape(-1) for fc in ("fc_avg_cf1", "fc_avg_cf2", "fc_max_cf1", "fc_max_cf2") for i in (0, 2)])
    want = cfen_oracle.cfsm2g({k: v.double() for k, v in sd.items()}, "c", *[x.double() for x in xs])
    ins = [G(nhwc(x), "x%d" % i) for i, x in enumerate(xs)] + [G(w, "gate weights")]
    out, ws = O((2, 12, 20, C), dtype, "out map"), _stats(2)
    ops.cfsm2g(*ins, C, out=out, stats_ws=ws)
    bands(out, ws, *ins)
    close(ops.from_nhwc(out, C), want, tol(dtype, 4))


# ---- tiling and ensemble --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 300), (127, 129)])
def test_tile_gather(u8, H, W):
    import tiling_ref as ref
    from test_hip_tiled import random_image
    T, o, B = 128, 16, 4
    a, img = random_image(H, W, H, u8)
    want = ref.gather(a, T, o, hwc=u8)
    ny, nx = ref.n_tiles(H, T, o), ref.n_tiles(W, T, o)
    n = ny * nx
    t0 = max(0, n - 1)                                     # the last batch: slot 0 is the last tile, the other slots are padded with copies of it
    gi = G(img, "image")
    slab = O((B, T, T, 3) if u8 else (B, 3, T, T), img.dtype, "input slab")
    if u8:
        byte_outputs_agree(lambda: ops.tile_gather(gi, T, ny, nx, t0, B, out=slab), [slab])
    else:
        ops.tile_gather(gi, T, ny, nx, t0, B, out=slab)
    bands(gi, slab)
    got = slab.cpu().numpy()
    assert all(np.array_equal(got[k], want[n - 1]) for k in range(B))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("H,W,B", [(70, 45, 8), (129, 383, 2)])
def test_tile_blend(dtype, H, W, B):
    """H * W = 3150 and 49407: no multiple of 4, so the float and the byte stores both end ragged"""
    from cfen_vit_dehazing_amd.util import util
    from test_hip_tiled import _blend_case
    T, o = 128, 16
    arena, ny, nx, want, cnt = _blend_case(H, W, T, o, dtype, B, 2)
    ga = G(arena, "arena")
    outs = [O((c, H, W), torch.float32, "blend out %d" % k) for k, c in enumerate((3, 1, 3))]
    ops.tile_blend(ga, B, T, H, W, ny, nx, o, out=outs)
    bands(ga, *outs)
    got = torch.cat(outs).cpu().numpy()
    assert np.abs(got - want).max() <= 2e-6
    out8 = [O((H, W, 3), torch.uint8, "blend u8 out %d" % k) for k in range(3)]
    byte_outputs_agree(lambda: ops.tile_blend(ga, B, T, H, W, ny, nx, o, output_u8=True, out=out8), out8)
    bands(ga)
    for img, plane in zip(out8, outs):
        assert np.array_equal(img.cpu().numpy(), util.tensor2im(plane.cpu()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_x8_expand_and_merge(dtype):
    import ensemble_ref as ref
    from cfen_vit_dehazing_amd.util import util
    from test_hip_ensemble import BAR, _arena, _arena_outputs, random_images, t_variant
    M, T = 1, 16
    for u8 in (True, False):
        a, img = random_images(2, T, T, u8)
        gi = G(img, "images")
        slab = O((8, T, T, 3) if u8 else (8, 3, T, T), img.dtype, "variant slab")
        if u8:
            byte_outputs_agree(lambda: ops.x8_expand(gi, 1, out=slab), [slab])
        else:
            ops.x8_expand(gi, 1, out=slab)
        bands(gi, slab)
        for i in range(8):
            assert torch.equal(slab[i], t_variant(img[1], i, hwc=u8))
    host = _arena(M, T, dtype, 7 * M + T)
    ga = G(host, "arena")
    flat = O((7 * M * T * T,), torch.float32, "merge out")
    got = ops.x8_merge(ga, M, T, out=flat)
    bands(ga, flat)
    for g, ys in zip(got, _arena_outputs(host, M, T)):
        want64 = np.stack([ref.merge(ys[m].double().numpy()) for m in range(M)])
        assert float(np.abs(g.cpu().numpy().astype(np.float64) - want64).max()) <= BAR
    # the uint8 form allocates its own outputs in the wrapper: through the C ABI, on guarded ones
    out8 = [O((M, T, T, 3), torch.uint8, "merge u8 out %d" % k) for k in range(3)]
    lib = _lib.load()
    byte_outputs_agree(lambda: check(lib.cfen_x8_merge(_lib.dtype_code(dtype), ptr(ga), M, T, 1, ptr(out8[0]), ptr(out8[1]), ptr(out8[2]), current_stream()),
                                     "x8_merge"), out8)
    bands(ga)
    for img, plane in zip(out8, got):
        assert np.array_equal(img[0].cpu().numpy(), util.tensor2im(plane[0].cpu()))


# ---- metrics and PNG ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["11x11", "37x53"])
def test_image_metrics(name):
    """uint8 and float input through the C ABI; scratch prefilled 0xff: its contents are irrelevant before the call"""
    import metrics_images as mi
    from test_hip_metrics import _check, _sse_slack
    fixture = np.load(os.path.join(GOLDEN, "metrics_pairs.npz"))
    a, b = mi.pair(name)
    Bn, H, W, _ = a.shape
    lib = _lib.load()
    nbytes = lib.cfen_image_metrics_bytes(Bn, 3, H, W)
    ta, tb = G(torch.from_numpy(a), "a uint8"), G(torch.from_numpy(b), "b uint8")
    scratch, out = O((max(nbytes, 8),), torch.uint8, "metrics scratch"), O((Bn, 2), torch.float64, "metrics out")
    check(lib.cfen_image_metrics(1, ptr(ta), ptr(tb), Bn, 3, H, W, 0.0, 1.0, ptr(scratch), ptr(out), current_stream()), "image_metrics")
    bands(ta, tb, scratch, out)
    _check("uint8", name, fixture, out[:, 0], out[:, 1])
    fa, fb = (G(torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)), "float input") for v in (a, b))
    out2 = O((Bn, 2), torch.float64, "metrics out (float input)")
    refill(scratch, "ff")
    check(lib.cfen_image_metrics(0, ptr(fa), ptr(fb), Bn, 3, H, W, 0.0, 1.0, ptr(scratch), ptr(out2), current_stream()), "image_metrics")
    bands(fa, fb, scratch, out2)
    _check("float32 range (0,1)", name, fixture, out2[:, 0], out2[:, 1], exact_sse=False, sse_slack=_sse_slack(a, b, 2.0 ** -24))
    assert torch.equal(out2[:, 1], out[:, 1])


@pytest.mark.parametrize("u8", [True, False])
def test_image_msssim(u8, golden_dir):
    import msssim_ref as mr
    from test_hip_msssim import _check
    name = "176x176"
    fixture = np.load(os.path.join(golden_dir, "msssim_pairs.npz"))
    a, b = mr.pair(name)
    Bn, H, W, _ = a.shape
    lib = _lib.load()
    nbytes = lib.cfen_image_msssim_bytes(Bn, 3, H, W)
    if u8:
        ta, tb = G(torch.from_numpy(a), "a"), G(torch.from_numpy(b), "b")
    else:
        ta, tb = (G(torch.from_numpy(np.ascontiguousarray(v.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255)), "float input") for v in (a, b))
    scratch, out = O((nbytes,), torch.uint8, "msssim scratch"), O((Bn, 11), torch.float64, "msssim out")
    check(lib.cfen_image_msssim(int(u8), ptr(ta), ptr(tb), Bn, 3, H, W, 0.0, 1.0, ptr(scratch), ptr(out), current_stream()), "image_msssim")
    bands(ta, tb, scratch, out)
    _check("uint8" if u8 else "float32 range (0,1)", name, fixture, out[:, 1:].reshape(Bn, 5, 2))


def test_png_deflate():
    """the two smallest images of png_ref's cases as a batch of 2 each: the stream up to its returned length equals the restatement's on an output
    prefilled 0xff and on one prefilled zero; the bytes past each stream's length keep their prefill"""
    import png_ref
    from cfen_vit_dehazing_amd import png
    for name in ("1x1", "Hx1"):
        img = png_ref.SMALL_CASES[name]()
        H, W, _ = img.shape
        other = np.ascontiguousarray(255 - img)
        gi = G(torch.from_numpy(np.stack([img, other])), "images")
        strip, stride = ctypes.c_size_t(0), ctypes.c_size_t(0)
        nbytes = _lib.load().cfen_png_workspace_bytes(2, H, W, ctypes.byref(strip), ctypes.byref(stride))
        assert stride.value == png.geometry(H, W)[4]
        slab, lengths = O((2, stride.value), torch.uint8, "png slab"), O((2,), torch.int32, "png lengths")
        work = O((max(nbytes, 16),), torch.uint8, "png workspace")

        def written(o):
            if o is lengths:
                return torch.ones(8, dtype=torch.bool, device=o.device)
            n = lengths.long()
            return (torch.arange(stride.value, device=o.device)[None] < n[:, None]).reshape(-1)

        byte_outputs_agree(lambda: ops.png_deflate(gi, out=slab, out_lengths=lengths, workspace=work), [slab, lengths], written)
        bands(gi, work)
        got, n = slab.cpu().numpy(), lengths.cpu().numpy()
        for k, im in enumerate((img, other)):
            assert 0 < n[k] <= stride.value and got[k, :n[k]].tobytes() == png_ref.stream(im), name


# ---- deformable convolution -----------------------------------------------------------------------------------------------------------------------
# Every entry point at the h/w-distinct geometries of tests/test_hip_dcn.py (HW_GEOMETRIES), through the C ABI, with the columns / backward scratch guarded
# and prefilled 0xff.  Bars: test_hip_dcn.py's (_out_close, _grads_close) against tests/dcn_ref.py in float64.  The v1 entry points take W before H.
@functools.lru_cache(maxsize=None)
def _dcn_problem(name, dtype):
    """x, w, off, mask, bias, gy on the host (float32 holding values of `dtype`), made once per geometry and dtype and never changed"""
    return _problem(*HW_GEOMETRIES[name], dtype, off_scale=1.5)


@functools.lru_cache(maxsize=None)
def _dcn_forward_ref(name, dtype, v2):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    x, w, off, mask, bias, _ = _dcn_problem(name, dtype)
    return dcn_ref.deform_conv_f64(x, off, w, s, p, d, groups, dg, **(dict(mask=mask, bias=bias) if v2 else {}))


@functools.lru_cache(maxsize=None)
def _dcn_backward_ref(name, dtype, v2):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    x, w, off, mask, bias, gy = _dcn_problem(name, dtype)
    return _ref_backward(x, off, w, gy, s, p, d, groups, dg, **(dict(mask=mask, bias=bias) if v2 else {}))


def _v1_geometry(name):
    """the integer arguments of the v1 entry points: W before H in every pair"""
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    return (B, C, H, W, Cout, k[1], k[0], s[1], s[0], p[1], p[0], d[1], d[0], groups, dg)


def _v2_geometry(name):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    return (B, C, H, W, Cout, k[0], k[1], s[0], s[1], p[0], p[1], d[0], d[1], groups, dg)


def _dcn_columns(name, dtype):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    n = int(_lib.load().cfen_deform_conv_columns_bytes(_lib.dtype_code(dtype), B, C, H, W, Cout, k[0], k[1], groups))
    return O((max(n, 16),), torch.uint8, "columns"), n


def _dcn_backward_scratch(name):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    Ho, Wo = dcn_ref.out_size(H, W, k, s, p, d)
    n = int(_lib.load().cfen_deform_conv_backward_bytes(B, C, H, W, Cout, k[0], k[1], Ho, Wo, groups))
    return O((max(n, 16),), torch.uint8, "backward scratch"), n


def _dcn_out(name, dtype):
    B, C, H, W, Cout, k, s, p, d, groups, dg = HW_GEOMETRIES[name]
    return O((B, Cout) + tuple(dcn_ref.out_size(H, W, k, s, p, d)), dtype, "output")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(HW_GEOMETRIES))
def test_deform_conv_forward(dtype, name):
    """cfen_deform_conv_forward on NCHW tensors (the NHWC copy and the tap-major weights go through the guarded columns; 6 channels per group: the NCHW gather)"""
    x, w, off, _, _, _ = _dcn_problem(name, dtype)
    lib, dt = _lib.load(), _lib.dtype_code(dtype)
    gx, gw, go = (G(t.to(dtype), n) for t, n in ((x, "input"), (w, "weight"), (off, "offset")))
    out = _dcn_out(name, dtype)
    columns, n = _dcn_columns(name, dtype)
    check(lib.cfen_deform_conv_forward(dt, ptr(gx), ptr(gw), ptr(go), ptr(out), *_v1_geometry(name), x.shape[0], ptr(columns), n, current_stream()),
          "deform_conv_forward")
    bands(gx, gw, go, out, columns)
    _out_close(out, {"float64": _dcn_forward_ref(name, dtype, False)}, dtype, "v1 forward")


def _takes_nhwc(name, dtype):
    """cfen_*_forward_nhwc need C / group to be a multiple of the 16-byte channel vector"""
    _, C, _, _, _, _, _, _, _, groups, _ = HW_GEOMETRIES[name]
    return (C // groups) % (4 if dtype == torch.float32 else 8) == 0


@pytest.mark.parametrize("name,dtype", [(n, dt) for n in HW_GEOMETRIES for dt in DTYPES if _takes_nhwc(n, dt)])
def test_deform_conv_forward_nhwc(name, dtype):
    """cfen_deform_conv_forward_nhwc and cfen_modulated_deform_conv_forward_nhwc: the input is a guarded [B][H][W][C] tensor the kernel samples from directly, the
    columns hold the weights only; at every geometry whose channels per group the entry points accept"""
    x, w, off, mask, bias, _ = _dcn_problem(name, dtype)
    lib, dt = _lib.load(), _lib.dtype_code(dtype)
    gx = G(x.permute(0, 2, 3, 1).contiguous().to(dtype), "input NHWC")
    gw, gb, go, gm = (G(t.to(dtype), n) for t, n in ((w, "weight"), (bias, "bias"), (off, "offset"), (mask, "mask")))
    out1, out2 = _dcn_out(name, dtype), _dcn_out(name, dtype)
    columns, n = _dcn_columns(name, dtype)
    check(lib.cfen_deform_conv_forward_nhwc(dt, ptr(gx), ptr(gw), ptr(go), ptr(out1), *_v1_geometry(name), x.shape[0], ptr(columns), n, current_stream()),
          "deform_conv_forward_nhwc")
    bands(gx, gw, go, out1, columns)
    _out_close(out1, {"float64": _dcn_forward_ref(name, dtype, False)}, dtype, "v1 forward (NHWC input)")
    refill(columns, "ff")
    check(lib.cfen_modulated_deform_conv_forward_nhwc(dt, ptr(gx), ptr(gw), ptr(gb), ptr(go), ptr(gm), ptr(out2), *_v2_geometry(name), 1, ptr(columns), n,
                                                      current_stream()), "modulated_deform_conv_forward_nhwc")
    bands(gx, gw, gb, go, gm, out2, columns)
    _out_close(out2, {"float64": _dcn_forward_ref(name, dtype, True)}, dtype, "v2 forward (NHWC input)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(HW_GEOMETRIES))
def test_deform_conv_backward(dtype, name):
    """cfen_deform_conv_backward_input (gradInput / gradOffset are overwritten: prefilled 0xff) and cfen_deform_conv_backward_parameters (gradWeight is
    accumulated into: it starts as zeros between bands), each on a backward scratch prefilled 0xff"""
    x, w, off, _, _, gy = _dcn_problem(name, dtype)
    lib, dt = _lib.load(), _lib.dtype_code(dtype)
    gx, gw, go, ggy = (G(t.to(dtype), n) for t, n in ((x, "input"), (w, "weight"), (off, "offset"), (gy, "grad_output")))
    grads = {"input": O(x.shape, dtype, "grad_input"), "offset": O(off.shape, dtype, "grad_offset"), "weight": O(w.shape, dtype, "grad_weight", fill="zero")}
    scratch, nb = _dcn_backward_scratch(name)
    check(lib.cfen_deform_conv_backward_input(dt, ptr(gx), ptr(go), ptr(ggy), ptr(grads["input"]), ptr(grads["offset"]), ptr(gw), *_v1_geometry(name),
                                              x.shape[0], ptr(scratch), nb, current_stream()), "deform_conv_backward_input")
    bands(gx, gw, go, ggy, scratch, grads["input"], grads["offset"])
    refill(scratch, "ff")
    check(lib.cfen_deform_conv_backward_parameters(dt, ptr(gx), ptr(go), ptr(ggy), ptr(grads["weight"]), *_v1_geometry(name), 1.0, x.shape[0], ptr(scratch),
                                                   nb, current_stream()), "deform_conv_backward_parameters")
    bands(gx, go, ggy, scratch, *grads.values())
    _grads_close(grads, {"float64": _dcn_backward_ref(name, dtype, False)}, dtype, "v1 backward")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(HW_GEOMETRIES))
def test_modulated_deform_conv(dtype, name):
    """cfen_modulated_deform_conv_forward and cfen_modulated_deform_conv_backward (h before w); grad_input / grad_offset / grad_mask are overwritten (prefilled
    0xff), grad_weight / grad_bias are accumulated into, so they start as zeros between bands"""
    x, w, off, mask, bias, gy = _dcn_problem(name, dtype)
    lib, dt = _lib.load(), _lib.dtype_code(dtype)
    ins = [G(t.to(dtype), n) for t, n in ((x, "input"), (w, "weight"), (bias, "bias"), (off, "offset"), (mask, "mask"))]
    gx, gw, gb, go, gm = ins
    out = _dcn_out(name, dtype)
    columns, n = _dcn_columns(name, dtype)
    check(lib.cfen_modulated_deform_conv_forward(dt, ptr(gx), ptr(gw), ptr(gb), ptr(go), ptr(gm), ptr(out), *_v2_geometry(name), 1, ptr(columns), n,
                                                 current_stream()), "modulated_deform_conv_forward")
    bands(out, columns, *ins)
    _out_close(out, {"float64": _dcn_forward_ref(name, dtype, True)}, dtype, "v2 forward")
    ggy = G(gy.to(dtype), "grad_output")
    grads = {"input": O(x.shape, dtype, "grad_input"), "offset": O(off.shape, dtype, "grad_offset"), "mask": O(mask.shape, dtype, "grad_mask"),
             "weight": O(w.shape, dtype, "grad_weight", fill="zero"), "bias": O((w.shape[0],), dtype, "grad_bias", fill="zero")}
    scratch, nb = _dcn_backward_scratch(name)
    check(lib.cfen_modulated_deform_conv_backward(dt, ptr(gx), ptr(gw), None, ptr(go), ptr(gm), ptr(grads["input"]), ptr(grads["weight"]), ptr(grads["bias"]),
                                                  ptr(grads["offset"]), ptr(grads["mask"]), ptr(ggy), *_v2_geometry(name), 1, ptr(scratch), nb,
                                                  current_stream()), "modulated_deform_conv_backward")
    bands(ggy, scratch, *ins, *grads.values())
    _grads_close(grads, {"float64": _dcn_backward_ref(name, dtype, True)}, dtype, "v2 backward")
