"""Every kernel instantiation and launch plan a tuning knob (csrc/cfen_tune_knobs.hpp) can select, against float64 math / the reference vectors.

SWEPT maps a knob's key to the values the GPU tests below run (they iterate these tuples); EXCLUDED maps the other keys to the reason they are not
run here.  tests/test_cabi.py::test_every_knob_is_swept_or_excused checks, without a GPU, that the two cover the library's table: a new knob row
fails there until someone tests or excuses it.

Bars are the ones of the default variants' own tests: tests/test_hip_ops.py::test_gemm_epilogues (tol 4 plain, 8 with bias + ReLU + residual + pos, 12 with
the folded LayerNorm), ::test_fused_mlp_block (6 / 10 / 6), and for the whole generator the helpers of tests/test_hip_net.py."""
import ctypes
import functools
import math
import os

import pytest
import torch

import cfen_oracle
from cfen_vit_dehazing_amd import _lib, ops, packing
from cfen_vit_dehazing_amd._lib import check, current_stream, dtype_code, ptr
from cfen_vit_dehazing_amd.manifest import synthetic_input
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from helpers import load_net_fixture
from test_hip_net import FP16_BAR, check_fp16_fixture, check_fp32_fixture, make_net
from test_hip_ops import DTYPES, close, dev, rnd, tol

pytestmark = pytest.mark.gpu

# ---- the ledger ---------------------------------------------------------------------------------------------------------------------------
DMA_FORCED = (2, 3, 4, 5, 12, 13, 14, 15, 22, 23, 24, 25, 7)     # k_gemm_dma through "gemm.kernel"; 7 has no case label: the `default:` arm, <T, 1, 4>
TILE_IDS = (2, 3, 4, 5, 12, 13, 14, 15, 22, 23, 24, 25, 32, 34, 45, 65)

OP_SWEPT = {
    "gemm.kernel": (0, 1) + DMA_FORCED,
    "gemm.small": TILE_IDS,                     # 32 / 34 / 45 / 65 are beyond "gemm.kernel"'s range: the shape rule reaches them
    "gemm.m128": (2, 32, 3, 4, 14, 34),
    "gemm.mid": (14,),
    "gemm.large": (3,),
    "gemm.nt": (1, 2),
    "gemm.defer_refill": (0,),
    "mlp.small_tiles": (0, 1, 2, 3, 4, 10, 11, 12, 20, 30, 40),
}
# launch-plan settings run on the whole generator: key -> values
NET_SWEPT = {
    "net.ln_fold": (0,),
    "net.embed_gather": (0,),
    "net.lvit_window": (0,),
    "net.fold_in_gemm": (0,),
    "net.attn_head_major": (0,),
    "net.fused_front_max_dim": (0, 96),
    "net.stream_front": (0, 1),
    "net.stream_mlp": (0, 1),
    "net.stream_mlp192": (0,),
    "net.gvit_chain": (0, 2, 3, 4, 5),
    "gvit.team": (7, 64),                       # not more: three blocks share the chip
    "tail.balance": (1,),
    "gemm.splitk": (1,),
    "gemm.small": (5, 25, 45),
    "gemm.m128": (2, 34),
    "gemm.nt": (2,),
    "mlp.small_tiles": (0, 21),
}
SWEPT = {k: tuple(dict.fromkeys(OP_SWEPT.get(k, ()) + NET_SWEPT.get(k, ()))) for k in list(OP_SWEPT) + [k for k in NET_SWEPT if k not in OP_SWEPT]}

_TIMING = "timing / debug setting: leaves work out or prints stamps and synchronises, results invalid on purpose"
EXCLUDED = {
    "gemm.splitk_stages": "read by no launcher (nothing calls its accessor); the row stays because tests/test_cabi.py pins the 61 keys",
    "mlp3.debug": _TIMING, "front3.debug": _TIMING, "lvit.debug": _TIMING, "gvit.debug": _TIMING, "tail.debug": _TIMING,
    "net.skip_classes": _TIMING, "net.skip_from": _TIMING, "net.skip_to": _TIMING, "net.extra_launches": _TIMING,
    "net.gvit_dummy_wgs": _TIMING, "net.gvit_dummy_us": _TIMING, "net.gvit_dummy_stream": _TIMING, "net.gvit_dummy_levels": _TIMING,
    "net.zero_memset": "1 has its test: test_hip_net.py::test_three_forwards_in_flight_on_replica_plans_match_single_forwards_bitwise",
    "mlp3.tm192": "swept by test_hip_ops.py::test_mlp_stream_block (24, 3, 4, 2, 25, 28 against the default and fp64)",
    "lvit.shape": "swept by test_hip_ops.py::test_lvit_window_block_against_oracle_and_unfused_chain (0, 1, 3, 4, 5, 6, 12, 13, 15; 8 / 9 are timing shapes)",
    "embed.defer_refill": "0 runs in test_hip_ops.py::test_embed_qkv_fused_front",
    "embed.lds": "swept by test_hip_ops.py::test_embed_qkv_fused_front (0, 3, 4)",
    "embed.stages": "swept by test_hip_ops.py::test_embed_qkv_fused_front (2, 3, 5 against 4)",
    "mlp3.pair": "0 and 1 run in test_hip_ops.py::test_mlp_stream_pair_kernel; 2 is the stamped timing build",
    "gemm.big": "6 runs in test_hip_ops.py::test_gemm_big_tile and ::test_gemm_big_tile_with_layernorm_folded",
    "gemm.big_min_tiles": "the threshold of \"gemm.big\": test_hip_ops.py::test_gemm_big_tile_with_layernorm_folded sets it",
    "gemm.splitk_release": "0 and 1 run in test_hip_ops.py::test_gemm_split_k_is_bit_reproducible_with_concurrent_lanes",
    "convT.tpw": "swept by test_hip_ops.py::test_multi_tile_workgroups_of_conv7_and_convT_cover_ragged_tile_counts",
    "conv7.tpw": "swept by test_hip_ops.py::test_multi_tile_workgroups_of_conv7_and_convT_cover_ragged_tile_counts",
    "conv.wlds": "0 / 2 run in test_hip_ops.py::test_conv_gather_with_and_without_lds_staged_weights_is_bitwise_equal",
    "conv.wlds_maxlog": "a pixel-count threshold between the two forms \"conv.wlds\" selects, which that test compares bitwise; it selects no kernel of its own",
    "attn.hm_pair": "swept by test_hip_ops.py::test_attention_head_major_layout",
    "dcn.tile": "swept by test_hip_dcn.py (k_dcn_lean against k_dcn_nhwc)",
    "dcn.tps": "swept by test_hip_dcn.py",
    "net.head5": "0 / 1 run in test_hip_net.py::test_head_from_input_and_fused_resblock_against_the_unfused_launches",
    "net.head_fused": "1 runs in test_hip_net.py::test_fused_head_equals_the_three_convolutions_bitwise",
    "net.resblock_fused": "1 runs in test_hip_net.py::test_head_from_input_and_fused_resblock_against_the_unfused_launches",
    "net.gvit_stream": "0 / 1 / 2 run in test_hip_net.py::test_two_lane_plan_equals_serial_plan_bitwise_full_size and its neighbours",
    "net.tail_fused": "0 / 1 / 2 run in test_hip_net.py::test_fused_tail_equals_the_separate_launches_bitwise",
    "tail.segments": "swept by test_hip_net.py::test_fused_tail_equals_the_separate_launches_bitwise",
    "net.up_fused": "1 runs in test_hip_net.py::test_gvit_upsampling_inside_the_fuse_conv_equals_the_upsample_launch",
    "net.keep_stages": "a parity-test switch (fused launches also store their stage maps); set by the tests of the fused tail and the chain plan",
    "gvit.max_concurrent": "caps the chain's team for forwards in flight: test_hip_net.py::test_three_forwards_in_flight_on_replica_plans_match_single_forwards_bitwise",
}


# ---- 1. token GEMM: tile and ring variants --------------------------------------------------------------------------------------------------
def ksteps(dtype, n):
    """K of n K-steps: one step is 128 bytes"""
    return n * (32 if dtype == torch.float32 else 64)


# (M, N, K-steps): K below, inside and twice around the deepest ring (8 stages); every M ragged against the 32 / 64 / 96 / 128-token tiles, every N against 96 and 16
COMBOS = ((1, 4, 1), (33, 100, 3), (130, 200, 9), (257, 100, 17))
COMBOS_BIG_M = ((130, 200, 1), (257, 100, 17), (130, 4, 3), (257, 200, 9))          # M > 128: the shape rule's "gemm.small" branch, not k_gemm_skinny
COMBOS_M128 = ((1, 4, 1), (33, 100, 3), (33, 200, 17), (1, 100, 9))                 # M <= 128: "gemm.m128"
S_POS = 16
# the tile id whose kernel differs from this id's in ring depth only (or not at all: 12 / 22 / 13 / 23 / 24 repeat an instantiation, 7 is 25's)
SAME_TILE = {12: 2, 22: 2, 32: 2, 13: 3, 23: 3, 14: 4, 24: 4, 34: 4, 15: 5, 25: 5, 45: 5, 65: 5, 7: 5}


@functools.lru_cache(maxsize=None)
def gemm_case(dtype, M, N, ks):
    """operands (on the device) and the float64 results of one shape, made once: x, w, bias, res, pos, plain, bias + ReLU + residual + pos"""
    K = ksteps(dtype, ks)
    x, w = rnd((M, K), 1, dtype), rnd((N, K), 2, dtype, 1 / math.sqrt(K))
    bias, res, pos = rnd((N,), 3, torch.float32), rnd((M, N), 4, dtype), rnd((S_POS, N), 5, dtype)
    ref = x.double() @ w.double().t()
    full = torch.relu(ref + bias.double()) + res.double() + pos.double()[torch.arange(M) % S_POS]
    d = dev()
    return x.to(d), w.to(d), bias.to(d), res.to(d), pos.to(d), ref, full


def run_gemm(dtype, M, N, ks, what):
    """plain and full-epilogue GEMM of a cached shape under the knobs in force, each against float64 at test_gemm_epilogues' bars -> (plain, full)"""
    x, w, bias, res, pos, ref, full = gemm_case(dtype, M, N, ks)
    plain = ops.gemm_nt(x, w)
    wp = close(plain, ref, tol(dtype, 4), "%s %dx%dx%d steps plain" % (what, M, N, ks))
    epi = ops.gemm_nt(x, w, bias=bias, residual=res, pos=pos, relu=True)
    we = close(epi, full, tol(dtype, 8), "%s %dx%dx%d steps bias+relu+res+pos" % (what, M, N, ks))
    print("%s %s M=%d N=%d K-steps=%d: plain %.2e, epilogue %.2e" % (what, str(dtype)[6:], M, N, ks, wp, we))
    return plain, epi


def same(a, b, what):
    assert all(torch.equal(p, q) for p, q in zip(a, b)), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kid", OP_SWEPT["gemm.kernel"])
def test_gemm_forced_kernel_ids(dtype, kid):
    """"gemm.kernel" = 0 (k_gemm_nt), 1 (k_gemm_skinny), every k_gemm_dma tile id in its range, and 7 (the switch's `default:` arm): float64 at all
    four shapes; ids that name the same tile run the same MFMA sequence per output element whatever the ring depth, so they are bitwise equal"""
    for M, N, ks in COMBOS:
        with ops.tuning({"gemm.kernel": kid}):
            got = run_gemm(dtype, M, N, ks, "gemm.kernel %d" % kid)
        if kid in SAME_TILE:
            with ops.tuning({"gemm.kernel": SAME_TILE[kid]}):
                same(got, run_gemm(dtype, M, N, ks, "gemm.kernel %d" % SAME_TILE[kid]), "gemm.kernel %d differs from %d" % (kid, SAME_TILE[kid]))


@functools.lru_cache(maxsize=None)
def ln_case(dtype, M, N, ks):
    """rows of mean 1 and spread 2, as test_gemm_with_layernorm_folded draws them"""
    D = ksteps(dtype, ks)
    x = rnd((M, D), 1, dtype, 2.0) + 1.0
    w = rnd((N, D), 2, torch.float32, D ** -0.5)
    g, b, bias = 1 + 0.1 * rnd((D,), 3, torch.float32), 0.1 * rnd((D,), 4, torch.float32), rnd((N,), 5, torch.float32)
    want = cfen_oracle.layer_norm(x.double(), g.double(), b.double()) @ w.double().t() + bias.double()
    f = packing.ln_folded(None, g, b, bias, "l", dtype, w)
    d = dev()
    return x.to(d), f["l.wl"].to(d), f["l.s"].to(d), f["l.bl"].to(d), want


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sid", OP_SWEPT["gemm.small"])
def test_gemm_small_rule_tile_ids(dtype, sid):
    """every tile id through the shape rule's few-tile branch ("gemm.small"; the only road to 32, 34, 45, 65): plain and with the epilogue at M > 128,
    and with a folded LayerNorm (which ignores "gemm.kernel" and never takes k_gemm_skinny) at every M; bitwise equal to the tile's shallowest ring"""
    base = SAME_TILE.get(sid)
    for M, N, ks in COMBOS_BIG_M:
        with ops.tuning({"gemm.small": sid}):
            got = run_gemm(dtype, M, N, ks, "gemm.small %d" % sid)
        if base:
            with ops.tuning({"gemm.small": base}):
                same(got, run_gemm(dtype, M, N, ks, "gemm.small %d" % base), "gemm.small %d differs from %d" % (sid, base))
    for M, N, ks in COMBOS:
        x, wl, s, bl, want = ln_case(dtype, M, N, ks)
        worst = {}
        for relu in (False, True):
            with ops.tuning({"gemm.small": sid}):
                got = ops.gemm_ln(x, wl, s, bl, relu=relu)
            worst[relu] = close(got, want.relu() if relu else want, tol(dtype, 12), "gemm.small %d folded LayerNorm %dx%dx%d steps" % (sid, M, N, ks))
            if base:
                with ops.tuning({"gemm.small": base}):
                    assert torch.equal(got, ops.gemm_ln(x, wl, s, bl, relu=relu)), "gemm.small %d differs from %d with a folded LayerNorm" % (sid, base)
        print("gemm.small %d %s folded LayerNorm M=%d N=%d K-steps=%d: %.2e, with ReLU %.2e" % (sid, str(dtype)[6:], M, N, ks, worst[False], worst[True]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mid", OP_SWEPT["gemm.m128"])
def test_gemm_m128_tile_ids(dtype, mid):
    """"gemm.m128": problems of <= 128 tokens on a k_gemm_dma tile instead of k_gemm_skinny"""
    for M, N, ks in COMBOS_M128:
        with ops.tuning({"gemm.m128": mid}):
            got = run_gemm(dtype, M, N, ks, "gemm.m128 %d" % mid)
        if mid in SAME_TILE:
            with ops.tuning({"gemm.m128": SAME_TILE[mid]}):
                same(got, run_gemm(dtype, M, N, ks, "gemm.m128 %d" % SAME_TILE[mid]), "gemm.m128 %d differs from %d" % (mid, SAME_TILE[mid]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_rule_boundaries_mid_and_large(dtype):
    """N = 200 is three feature tiles.  M = 5443 is 171 tiles of 32 tokens: 513 tiles, the first count past "gemm.small"'s 512 -> "gemm.mid";
    M = 21827 is 342 tiles of 64 tokens: 1026 >= 1024 -> "gemm.large".  Each once with a tile that is not its default, and one step below the boundary
    the knob must not matter.  (The bitwise comparison with the tile forced through "gemm.kernel" cannot prove which tile ran -- tiles of another height
    add the same products in the same K order, and an operator call has no launch record to read; what holds is the float64 bar on the kernel the rule
    picked, whichever it was.  The launch-plan tests below read the kernel names.)"""
    (mid,), (large,) = OP_SWEPT["gemm.mid"], OP_SWEPT["gemm.large"]
    with ops.tuning({"gemm.mid": mid}):
        at = run_gemm(dtype, 5443, 200, 3, "gemm.mid %d" % mid)
        below = run_gemm(dtype, 5440, 200, 3, "gemm.mid %d, 510 tiles" % mid)
    with ops.tuning({"gemm.kernel": mid}):
        same(at, run_gemm(dtype, 5443, 200, 3, "gemm.kernel %d" % mid), "gemm.mid %d at 513 tiles differs from the forced tile" % mid)
    same(below, run_gemm(dtype, 5440, 200, 3, "default"), "gemm.mid reaches below its boundary")
    with ops.tuning({"gemm.large": large}):
        at = run_gemm(dtype, 21827, 200, 3, "gemm.large %d" % large)
        below = run_gemm(dtype, 21760, 200, 3, "gemm.large %d, 1020 tiles" % large)
    with ops.tuning({"gemm.kernel": large}):
        same(at, run_gemm(dtype, 21827, 200, 3, "gemm.kernel %d" % large), "gemm.large %d at 1026 tiles differs from the forced tile" % large)
    same(below, run_gemm(dtype, 21760, 200, 3, "default"), "gemm.large reaches below its boundary")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("knob,value", [("gemm.nt", v) for v in OP_SWEPT["gemm.nt"]] + [("gemm.defer_refill", v) for v in OP_SWEPT["gemm.defer_refill"]])
def test_gemm_data_movement_knobs_are_bitwise_neutral(dtype, knob, value):
    """non-temporal weight DMAs and the refill's place in the K-step move the same bytes into the same LDS slots: float64 bar and the default's bits,
    on every k_gemm_dma tile id ("gemm.nt" 1 covers M <= 512 only: both shapes are below)"""
    for route, ids, combos in (("gemm.kernel", DMA_FORCED, COMBOS[1:]), ("gemm.small", (32, 34, 45, 65), COMBOS_BIG_M[1:3])):
        for tid in ids:
            for M, N, ks in combos:
                with ops.tuning({route: tid}):
                    want = run_gemm(dtype, M, N, ks, "%s %d" % (route, tid))
                    with ops.tuning({knob: value}):
                        got = run_gemm(dtype, M, N, ks, "%s %d, %s %d" % (route, tid, knob, value))
                same(got, want, "%s %d changes the bits of tile id %d" % (knob, value, tid))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route,tid", [("gemm.kernel", t) for t in DMA_FORCED] + [("gemm.small", t) for t in (32, 34, 45, 65)])
def test_embed_gather_under_every_dma_tile_id(dtype, route, tid):
    """the patch gather inside k_gemm_dma's loader (C = 48, p = 2: D = 192, three fp16 / six fp32 K-steps; 576 tokens: ragged against the 128-token tile)
    against patchify followed by a float64 GEMM, at test_embed_gather_equals_patchify_then_gemm's bar"""
    d = dev()
    B, C, H, W, ws, p = 3, 48, 16, 48, 16, 2
    D, S = 4 * C, (ws // p) ** 2
    fmap = ops.to_nhwc(rnd((B, C, H, W), 1, dtype)).to(d)
    w = rnd((D, D), 2, dtype, 1 / math.sqrt(D)).to(d)
    b = rnd((D,), 3, torch.float32, 0.1).to(d)
    pos = rnd((S, D), 4, dtype).to(d)
    tok = ops.patchify(fmap, C, ws, p).double().cpu()
    ref = tok @ w.double().cpu().t() + b.double().cpu() + tok + pos.double().cpu().repeat(tok.shape[0] // S, 1)
    with ops.tuning({route: tid}):
        got = ops.embed_gather(fmap, C, ws, p, w, b, pos)
    print("embed_gather %s %d %s: %.2e" % (route, tid, str(dtype)[6:], close(got, ref, tol(dtype, 4), "embed_gather under %s %d" % (route, tid))))
    if tid in SAME_TILE:
        with ops.tuning({route: SAME_TILE[tid]}):
            assert torch.equal(got, ops.embed_gather(fmap, C, ws, p, w, b, pos)), "gather: tile id %d differs from %d" % (tid, SAME_TILE[tid])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("family,kid", [("nt", 0), ("skinny", 1), ("dma", 15), ("dma deep ring", 25), ("big", 6)])
def test_gemm_padded_leading_dimensions(dtype, family, kid):
    """ldx > K, ldw > K, ldy > N, ldr > N through the C ABI (ops.gemm_nt passes the tight ones): every padding element is NaN, so one read of it poisons
    the result; the padding columns of Y must come back bit-untouched"""
    M, N, ks = 130, 200, 3
    x, w, bias, res, pos, ref, full = gemm_case(dtype, M, N, ks)
    K = x.shape[1]
    d = dev()

    def padded(t, ld):
        buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=d)
        buf[:, :t.shape[1]] = t
        return buf

    ldx, ldw, ldy, ldr = K + 16, K + 32, N + 8, N + 12
    X, W, R, Y = padded(x, ldx), padded(w, ldw), padded(res, ldr), torch.full((M, ldy), float("nan"), dtype=dtype, device=d)
    ibits = torch.int32 if dtype == torch.float32 else torch.int16
    before = Y.view(ibits)[:, N:].clone()
    with ops.tuning({"gemm.kernel": kid}):
        check(_lib.load().cfen_gemm_nt(dtype_code(dtype), ptr(X), ldx, ptr(W), ldw, ptr(bias), ptr(R), ldr, ptr(pos), S_POS, ptr(Y), ldy, M, N, K, 1,
                                       current_stream()), "gemm_nt")
    torch.cuda.synchronize()
    print("padded leading dimensions, %s %s: %.2e" % (family, str(dtype)[6:], close(Y[:, :N], full, tol(dtype, 8), family)))
    assert torch.equal(Y.view(ibits)[:, N:], before), "%s: the padding columns of Y were written" % family
    with ops.tuning({"gemm.kernel": kid}):
        assert torch.equal(Y[:, :N], ops.gemm_nt(x, w, bias=bias, residual=res, pos=pos, relu=True)), "%s: padded and tight calls differ" % family


# ---- 2. fused MLP tilings -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mlp_case(dtype, D, H, M):
    """test_fused_mlp_block's operands and float64 results, made once per shape"""
    x = rnd((M, D), 1, dtype)
    g, b = 1 + 0.1 * rnd((D,), 2, torch.float32), 0.1 * rnd((D,), 3, torch.float32)
    w1a, w2a = rnd((H, D), 4, dtype, D ** -0.5), rnd((D, H), 5, dtype, 0.5 * H ** -0.5)
    w1b, w2b = rnd((H, D), 6, dtype, D ** -0.5), rnd((D, H), 7, dtype, 0.5 * H ** -0.5)
    b1a, b2a, b1b, b2b = (0.1 * rnd((n,), 8 + i, torch.float32) for i, n in enumerate((H, D, H, D)))
    att, wp = rnd((M, D), 12, dtype), rnd((D, D), 13, dtype, D ** -0.5)
    xd = x.double()
    ffn = lambda v, w1, b1, w2, b2, ln: v + torch.relu((cfen_oracle.layer_norm(v, g.double(), b.double()) if ln else v) @ w1.double().t()
                                                       + b1.double()) @ w2.double().t() + b2.double()
    y1 = ffn(xd, w1a, b1a, w2a, b2a, True)
    y2 = ffn(y1, w1b, b1b, w2b, b2b, False)
    nol = ffn(xd, w1a, b1a, w2a, b2a, False)
    prj = ffn(xd + att.double() @ wp.double().t(), w1a, b1a, w2a, b2a, True)
    d = dev()
    if dtype == torch.float16:
        kd, kh = packing.kperm32(D), packing.kperm32(H)
        pk = lambda w1, w2: (w1[:, kd].contiguous().to(d), w2[:, kh].contiguous().to(d))
    else:
        pk = lambda w1, w2: (w1.to(d), w2.to(d))
    dv = dict(x=x.to(d), ln=(g.to(d), b.to(d)), a=pk(w1a, w2a), b=pk(w1b, w2b), b1a=b1a.to(d), b2a=b2a.to(d), b1b=b1b.to(d), b2b=b2b.to(d),
              proj=(att.to(d), wp.to(d)))
    return dv, y1, y2, nol, prj


@pytest.mark.parametrize("D", [96, 192])
@pytest.mark.parametrize("dtype,small", [(dt, v) for dt in DTYPES for v in OP_SWEPT["mlp.small_tiles"] if v < 10 or dt == torch.float16])
def test_fused_mlp_tilings(dtype, small, D):
    """the body of test_fused_mlp_block (same float64 reference, optional parts and bars) under every "mlp.small_tiles": 0 .. 4 the five k_mlp tilings per
    width (both dtypes), >= 10 the k_mlp2 forms (fp16; tens digit D = 96, ones digit D = 192); M ragged against the 64- to 512-token workgroups.  The
    projection prologue at test_mlp_block_with_projection_prologue's bar.  The fold epilogue is bitwise unpatchify of the value's own token-major result."""
    for M in (64, 130, 300):
        for H in (2 * D, 4 * D):
            v, y1, y2, nol, prj = mlp_case(dtype, D, H, M)
            with ops.tuning({"mlp.small_tiles": small}):
                one = ops.mlp_block(v["x"], v["a"][0], v["b1a"], v["a"][1], v["b2a"], ln=v["ln"])
                two = ops.mlp_block(v["x"], v["a"][0], v["b1a"], v["a"][1], v["b2a"], ln=v["ln"], second=(v["b"][0], v["b1b"], v["b"][1], v["b2b"]))
                no = ops.mlp_block(v["x"], v["a"][0], v["b1a"], v["a"][1], v["b2a"])
                pr = ops.mlp_block(v["x"], v["a"][0], v["b1a"], v["a"][1], v["b2a"], ln=v["ln"], proj=v["proj"])
            what = "mlp.small_tiles %d D=%d H=%d M=%d " % (small, D, H, M)
            worst = (close(one, y1, tol(dtype, 6), what + "stage a"), close(two, y2, tol(dtype, 10), what + "both stages"),
                     close(no, nol, tol(dtype, 6), what + "no LN"), close(pr, prj, tol(dtype, 8), what + "projection prologue"))
            print(what + str(dtype)[6:] + ": stage a %.2e, both %.2e, no LN %.2e, projection %.2e" % worst)
    # fold epilogue (test_fused_mlp_fold_epilogue's geometry: 8x8 windows of 2x2 patches on a 16x32 map, padded channel stride; D = 4 C)
    B, C, Hm, Wm, ws, pp = 2, D // 4, 16, 32, 8, 2
    cs, H, M = C + 8, 2 * D, B * Hm * Wm // 4
    x = rnd((M, D), 1, dtype)
    w1, w2 = rnd((H, D), 2, dtype, D ** -0.5), rnd((D, H), 3, dtype, H ** -0.5)
    b1, b2 = 0.1 * rnd((H,), 4, torch.float32), 0.1 * rnd((D,), 5, torch.float32)
    d = dev()
    if dtype == torch.float16:
        w1, w2 = w1[:, packing.kperm32(D)].contiguous(), w2[:, packing.kperm32(H)].contiguous()
    with ops.tuning({"mlp.small_tiles": small}):
        tok = ops.mlp_block(x.to(d), w1.to(d), b1.to(d), w2.to(d), b2.to(d))
        fm = ops.mlp_block(x.to(d), w1.to(d), b1.to(d), w2.to(d), b2.to(d), fold=(B, Hm, Wm, C, cs, ws, pp))
    assert torch.equal(fm, ops.unpatchify(tok, B, Hm, Wm, C, cs, ws, pp))


# ---- 4. launch-plan knobs on the whole generator --------------------------------------------------------------------------------------------------
# Fixtures, smallest first: "tiny" = tiny_nf24_hdr4 (64 px, batch 2) serves most settings; "w32" = cfs_full256_nf24_hdr4 (batch 1) has the 32-pixel windows
# that k_lvit_window and the D = 384 stream kernels need.  A setting is run on the smallest one on which it changes the sequence of kernel names.
# Kinds of net: fp32, fp16, and "chain" = fp16 with the GViT weights also packed as fragment streams, which "net.gvit_chain" / "gvit.team" need to act at all.
FIXTURES = {"tiny": "tiny_nf24_hdr4", "w32": "cfs_full256_nf24_hdr4", "full512": "full512_nf24_hdr4"}      # (full512: only where a needed kernel runs on neither)
PLAN_FIXTURES = ("tiny", "w32")
CHAIN_KEYS = ("net.gvit_chain", "gvit.team")
NET_CASES = [(key, value, kind) for key, values in NET_SWEPT.items() for value in values for kind in (("chain",) if key in CHAIN_KEYS else ("fp32", "fp16"))]
# Settings that change the sequence of kernel NAMES on no fixture in the tree, so the names cannot show that they acted: (the kernel a fixture's default plan
# must launch for the setting to reach any code, or None where it reaches none; the reason).  test_settings_that_keep_the_kernel_names runs them all the same.
_FP16_ONLY = (None, "selects between fp16-only kernels (k_lvit_window, k_front3, k_mlp3, k_attention_hm): an fp32 net launches the same kernels either way")
_NT = ("k_gemm_dma", "the DMA policy is an argument of the same k_gemm_dma instantiations; data movement only, so bitwise the default plan's outputs")
_SPLITK = ("k_gemm_dma", "the K slices are a grid dimension of the k_gemm_dma instantiation the tile-major GViT weights take anyway")
_TEAM = ("k_gvit_chain", "the team is the grid of the same k_gvit_chain (and sets how K is split per phase): other summation order, same kernel")
NET_DEAD = {
    ("net.lvit_window", 0, "fp32"): _FP16_ONLY, ("net.attn_head_major", 0, "fp32"): _FP16_ONLY,
    ("net.stream_front", 0, "fp32"): _FP16_ONLY, ("net.stream_front", 1, "fp32"): _FP16_ONLY,
    ("net.stream_mlp", 0, "fp32"): _FP16_ONLY, ("net.stream_mlp", 1, "fp32"): _FP16_ONLY, ("net.stream_mlp192", 0, "fp32"): _FP16_ONLY,
    ("mlp.small_tiles", 21, "fp32"): (None, "fp32 has no k_mlp2: 21 takes the tilings the default 10 takes (launch_mlp: >= 3 at D = 96, the `small ?` arm at D = 192)"),
    ("gemm.splitk", 1, "fp32"): _SPLITK, ("gemm.splitk", 1, "fp16"): _SPLITK,
    ("gemm.nt", 2, "fp32"): _NT, ("gemm.nt", 2, "fp16"): _NT,
    ("gvit.team", 7, "chain"): _TEAM, ("gvit.team", 64, "chain"): _TEAM,
    ("tail.balance", 1, "fp32"): (None, "k_tail_fused is fp16 only"),
    ("tail.balance", 1, "fp16"): ("k_tail_fused", "which wave group scales / stores the 7x7's rows is an argument of the same k_tail_fused"),
}
BITWISE_IN_NET = ("gemm.nt",)          # data movement only: the outputs are the default plan's bits


class Plans:
    """one built net per (fixture, kind), with its input, its default plan's outputs and kernel names"""

    def __init__(self):
        self.built = {}

    def get(self, fixture, kind):
        if (fixture, kind) not in self.built:
            cfg, batch, z = load_net_fixture(FIXTURES[fixture])
            if kind == "chain":
                os.environ["CFEN_GVIT_CHAIN"] = "1"          # read when the net is built (hipnet.dec_ipt): the GViT weights are packed as fragment streams too
            try:
                net = make_net(cfg, "fp32" if kind == "fp32" else "fp16")
            finally:
                os.environ.pop("CFEN_GVIT_CHAIN", None)
            assert net.gvit_chain == (kind == "chain")
            x = synthetic_input(batch, cfg).to("cuda:0")
            outs = [o.clone() for o in net(x)]
            self.check(fixture, kind, net, z, outs)
            self.built[fixture, kind] = (net, x, z, outs, self.kernels(net, x))
        return self.built[fixture, kind]

    @staticmethod
    def kernels(net, x):
        return [l[4] for l in net.profile(x)["launches"]]

    @staticmethod
    def check(fixture, kind, net, z, outs):
        """the bars of the fixture's own test (tests/test_hip_net.py)"""
        if kind == "fp32":
            return max(check_fp32_fixture(FIXTURES[fixture], net, z, outs))
        return check_fp16_fixture(z, outs)

    def run(self, fixture, kind, key, value):
        """a forward under the setting: checked against the fixture and the default plan -> (the kernel sequence differs, worst error against the fixture, max-abs distance from the default plan's outputs)"""
        net, x, z, base, names = self.get(fixture, kind)
        with ops.tuning({key: value}):
            outs = [o.clone() for o in net(x)]
            worst = self.check(fixture, kind, net, z, outs)
            differs = self.kernels(net, x) != names
        if kind == "chain":
            assert net.chain_errors() == [0, 0, 0]
        apart = max(float((a - b).abs().max()) for a, b in zip(outs, base))
        assert apart <= FP16_BAR, "%s = %d: outputs differ from the default plan's by %.3e" % (key, value, apart)
        return differs, worst, apart


@pytest.fixture(scope="module")
def plans():
    p = Plans()
    yield p
    p.built.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("key,value,kind", [c for c in NET_CASES if c not in NET_DEAD])
def test_launch_plan_setting_on_the_whole_generator(plans, key, value, kind):
    """every stage and output of a forward under the setting against the reference vectors, at the bars the default plan is held to, and against the
    default plan's outputs; the setting is not vacuous: on one of the fixtures the sequence of kernels differs from the default plan's"""
    for fixture in PLAN_FIXTURES:
        differs, worst, apart = plans.run(fixture, kind, key, value)
        print("%s = %d, %s on %s: worst %.2e, from the default plan %.2e, kernel sequence %s" % (key, value, kind, fixture, worst, apart,
                                                                                               "differs" if differs else "as the default plan's"))
        if differs:
            return
    raise AssertionError("%s = %d launches the default plan's kernels on every fixture (%s): the test would be blind -- list it in NET_DEAD" % (key, value, kind))


@pytest.mark.parametrize("key,value,kind", list(NET_DEAD))
def test_settings_that_keep_the_kernel_names(plans, key, value, kind):
    """NET_DEAD is checked, not believed: under each of its settings the kernel names ARE the default plan's on every fixture tried, and the forward holds the
    same bars.  Where the setting acts through an argument of a kernel, the run is on the smallest fixture whose plan launches that kernel (else it would reach
    no code): the ragged and the large chain team, the 7x7's other wave split, non-temporal weight DMAs (bitwise), in-launch split-K."""
    needs, _ = NET_DEAD[key, value, kind]
    reached = needs is None
    for fixture in FIXTURES if needs else PLAN_FIXTURES:
        names = plans.get(fixture, kind)[4]
        differs, worst, apart = plans.run(fixture, kind, key, value)
        print("%s = %d, %s on %s: worst %.2e, from the default plan %.2e" % (key, value, kind, fixture, worst, apart))
        assert not differs, "%s = %d changes the kernel sequence on %s (%s): it belongs to the settings run by name, not in NET_DEAD" % (key, value, fixture, kind)
        if key in BITWISE_IN_NET:
            assert apart == 0.0, "%s = %d moves data only and changed the outputs by %.3e" % (key, value, apart)
        if needs and any(n.startswith(needs) for n in names):
            reached = True
            break
    assert reached, "no fixture launches %s: %s = %d was run blind" % (needs, key, value)
