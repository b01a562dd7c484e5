"""Value edges of the normalising, softmax and gate kernels on the GPU: rows / channels whose mean is up to 256 times their spread, a variance
near eps, constant rows, a common score offset of 1e3 .. 1e4, ties, a dominating key on either side of every key-block edge, saturated gates.
Inputs, float64 references and bars come from value_edges_ref.py (checked on the CPU by test_value_edges_host.py); every case prints its
error / bar ratio before the assertion."""
import math

import pytest
import torch
import torch.nn.functional as F

import cfen_oracle
import value_edges_ref as ve
from cfen_vit_dehazing_amd import ops, packing
from helpers import FP16_STAGE_MARGIN, knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from value_edges_ref import fold_operands, ln_operands

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.float16]


def dev():
    return torch.device("cuda:0")


def tol(dtype, scale=1.0):
    return (3e-5 if dtype == torch.float32 else 3e-3) * scale


def _report(what, dtype, ratios):
    """print every case's error / bar, then fail on those above 1"""
    print("%s %s: error / bar  %s" % (what, str(dtype).replace("torch.", ""), "  ".join("%s %.3g" % kv for kv in ratios.items())))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, "%s %s: error / bar above 1: %r" % (what, dtype, bad)


# ---------------------------------------------------------------------------------------------------
# statistics, single operators
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", [(5, 96), (33, 384), (7, 2048)])
def test_layernorm_value_edges(dtype, M, D):
    g, b = ln_operands(D)
    ratios = {}
    for case in ve.CASES:
        x = ve.rows(case, M, D, dtype)
        want = ve.layernorm(x, g, b, torch.float64)
        e32 = ve.e32_of(ve.layernorm(x, g, b, torch.float32), want)
        ratios[case] = ve.ratio(ops.layernorm(x.to(dev()), g.to(dev()), b.to(dev())), want, e32, dtype)
    _report("layernorm (%d, %d)" % (M, D), dtype, ratios)


def _folded(run, what, dtype, M, K, N):
    wl, s, bl = fold_operands(K, N, dtype)
    d = dev()
    ratios = {}
    for case in ve.CASES:
        x = ve.rows(case, M, K, dtype)
        want = ve.gemm_ln(x, wl, s, bl, torch.float64)
        e32 = ve.e32_of(ve.gemm_ln(x, wl, s, bl, torch.float32), want)
        ratios[case] = ve.ratio(run(x.to(d), wl.to(d), s.to(d), bl.to(d)), want, e32, dtype)
    _report("%s (M %d, K %d, N %d)" % (what, M, K, N), dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D,N,big", [(100, 384, 96, 0), (33, 1536, 96, 0), (33, 1536, 96, 1), (33, 384, 768, 1)])
def test_gemm_ln_value_edges(dtype, M, D, N, big):
    """the LayerNorm-folded GEMM on the packed operands; big: under the big-tile kernel id ("gemm.big" 6 with "gemm.big_min_tiles" 1).  The shape
    rule gives 192 x 128 tiles to N >= 768 only, so (33, 1536, 96) runs the 96 x 32 kernel under either setting; (33, 384, 768) is there to put
    the statistics of the big-tile instantiation itself under the same rows.

    fp32 at (33, 1536, 96), measured on an MI355X (error / bar):
                 rho0   rho1   rho8   rho64  rho256  tiny_std  constant  alt_sign
      one-pass   0.724  0.965  1.08   9.41   30.6    11.6      0.792     7.07       (E[x^2] - mean^2, one accumulator chain over K)
      shifted    0.882  0.965  1.08   1.19   1.14    1.14      0.792     0.737      (shifted sums, one accumulator chain over K)
      as shipped 0.739  0.322  0.22   0.291  0.298   0.266     0.221     0.219      (shifted sums, chunks of 16 products summed from zero)
    The middle row was the plain product's own error: x wl^T from the same kernel with float64 mean and variance gave the same figures to three
    digits -- a single chain of 1536 dependent fp32 MFMA additions, 3 .. 5 times further from float64 than the CPU's blocked product."""
    with ops.tuning({"gemm.big_min_tiles": 1, "gemm.big": 6} if big else {}):
        _folded(lambda x, wl, s, bl: ops.gemm_ln(x, wl, s, bl), "gemm_ln%s" % (" big tile" if big else ""), dtype, M, D, N)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K,nsplit", [(33, 96, 256, 2), (128, 96, 1536, 4)])
def test_gemm_splitk_folded_value_edges(dtype, M, N, K, nsplit):
    """every K slice sums its part of the row, the reducer adds the slices' sums: the statistics must survive that too"""
    _folded(lambda x, wl, s, bl: ops.gemm_splitk(x, wl, nsplit, bias=bl, lnf_s=s), "gemm_splitk x%d folded" % nsplit, dtype, M, K, N)


def test_gemm_chain_folded_phase_value_edges():
    M, N, K = 16, 128, 64                                   # the smallest shape test_gemm_chain_single_phase runs

    def run(x, wl, s, bl):
        y = torch.full((M, N), float("nan"), dtype=torch.float16, device=dev())
        assert ops.gemm_chain([dict(x=x, w=wl, y=y, bias=bl, lnf_s=s)], M, 3) == 0
        return y
    _folded(run, "gemm_chain folded phase", torch.float16, M, K, N)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,H,W", [(2, 24, 32, 32), (1, 8, 64, 64)])
def test_instnorm_relu_value_edges(dtype, B, C, H, W):
    """every channel its own case (value_edges_ref.channels)"""
    x, names = ve.channels(B, C, H, W, dtype)
    want = ve.instnorm_relu(x, torch.float64)
    r32 = ve.instnorm_relu(x, torch.float32)
    got = ops.from_nhwc(ops.instnorm_relu_(ops.to_nhwc(x).to(dev()), C), C).cpu()
    ratios = {}
    for case in ve.CASES:
        ch = [c for c, n in enumerate(names) if n == case]
        ratios[case] = ve.ratio(got[:, ch], want[:, ch], ve.e32_of(r32[:, ch], want[:, ch]), dtype)
    _report("instnorm_relu (%d, %d, %d, %d)" % (B, C, H, W), dtype, ratios)


def _cfsm_operands(C, dtype):
    """all-negative maps whose sum has channel 1 at mean -256 and unit spread; the gates' second matrices scaled so that the largest
    pre-sigmoid value is exactly +-200 (expf(200) overflows fp32: the gate must come out 0 or 1, not NaN)"""
    B, H, W = 2, 32, 32
    g = torch.Generator().manual_seed(700 + C)
    xs = [-(torch.randn(B, C, H, W, generator=g, dtype=torch.float64).abs() + 0.1) for _ in range(3)]
    z = ve.rows("rho0", B, H * W, torch.float64, seed=5).view(B, H, W)
    xs[0][:, 1], xs[1][:, 1], xs[2][:, 1] = z - 250.0, torch.full((B, H, W), -3.0, dtype=torch.float64), torch.full((B, H, W), -3.0, dtype=torch.float64)
    xs = [x.to(dtype) for x in xs]
    h = C // 4
    names = ("fc_avg_cf1", "fc_avg_cf2", "fc_max_cf1", "fc_max_cf2")
    sd = {}
    for fc in names:
        sd["c.%s.0.weight" % fc] = torch.randn(h, C, 1, 1, generator=g) / math.sqrt(C)
        sd["c.%s.2.weight" % fc] = torch.randn(C, h, 1, 1, generator=g) / math.sqrt(h)
    comb = xs[0].double() + xs[1].double() + xs[2].double()
    avg, mx = comb.mean((2, 3), keepdim=True), comb.amax((2, 3), keepdim=True)
    fc = lambda n, v: F.conv2d(torch.relu(F.conv2d(v, sd["c.%s.0.weight" % n].double())), sd["c.%s.2.weight" % n].double())
    for k in ("1", "2"):
        a = fc("fc_avg_cf" + k, avg) + fc("fc_max_cf" + k, mx)
        for n in ("fc_avg_cf" + k, "fc_max_cf" + k):
            sd["c.%s.2.weight" % n] = (sd["c.%s.2.weight" % n].double() * (200.0 / float(a.abs().max()))).float()
    w = torch.cat([sd["c.%s.%d.weight" % (fc_, i)].reshape(-1) for fc_ in names for i in (0, 2)])
    return xs, sd, w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 24])
def test_cfsm2g_value_edges(dtype, C):
    xs, sd, w = _cfsm_operands(C, dtype)
    want = cfen_oracle.cfsm2g({k: v.double() for k, v in sd.items()}, "c", *[x.double() for x in xs])
    r32 = cfen_oracle.cfsm2g(sd, "c", *[x.float() for x in xs])
    assert bool(torch.isfinite(want).all()) and float(want.max()) < 0
    d = dev()
    xn = [ops.to_nhwc(x).to(d) for x in xs]
    got = ops.from_nhwc(ops.cfsm2g(xn[0], xn[1], xn[2], w.to(d), C), C)
    _report("cfsm2g C %d" % C, dtype, {"negative_rho256_gates200": ve.ratio(got, want, ve.e32_of(r32, want), dtype)})


# ---------------------------------------------------------------------------------------------------
# statistics inside the fused MLP blocks (fp16): hidden activations and the result are stored in fp16, so the bar is the project's stage bar --
# FP16_STAGE_MARGIN times the distance between the float64 block with those stores rounded to fp16 and the exact float64 block
def _ffn64(x, g, b, w1, b1, w2, b2, quant):
    """cfen_oracle.vit_tokens, norm2 -> linear1 -> ReLU -> linear2 + residual, with its quant points"""
    y = cfen_oracle.layer_norm(x, g.double(), b.double())
    y = quant(torch.relu(y @ w1.double().t() + b1.double()))
    return quant(x + y @ w2.double().t() + b2.double())


def _mlp_value_edges(what, D, H, M, run):
    dt = torch.float16
    g, b = ln_operands(D)
    gen = torch.Generator().manual_seed(80)
    w1, w2 = (torch.randn(H, D, generator=gen) * D ** -0.5).to(dt), (torch.randn(D, H, generator=gen) * 0.5 * H ** -0.5).to(dt)
    b1, b2 = 0.1 * torch.randn(H, generator=gen), 0.1 * torch.randn(D, generator=gen)
    half = lambda t: t.to(dt).double()
    ratios = {}
    for rho in (0, 8, 64):
        x = ve.rows("rho%d" % rho, M, D, dt)
        exact = _ffn64(x.double(), g, b, w1, b1, w2, b2, lambda t: t)
        model = float((_ffn64(x.double(), g, b, w1, b1, w2, b2, half) - exact).abs().max())
        err = float((run(x, g, b, w1, b1, w2, b2).double().cpu() - exact).abs().max())
        ratios["rho%d" % rho] = err / (FP16_STAGE_MARGIN * model)
        print("%s rho %d: max-abs %.3e, rounding model %.3e, measured / model %.2f" % (what, rho, err, model, err / model))
    _report(what, dt, ratios)


@pytest.mark.parametrize("D,H,M", [(96, 384, 70), (192, 768, 130)])
def test_mlp_block_value_edges(D, H, M):
    d = dev()
    kd, kh = packing.kperm32(D), packing.kperm32(H)
    run = lambda x, g, b, w1, b1, w2, b2: ops.mlp_block(x.to(d), w1[:, kd].contiguous().to(d), b1.to(d), w2[:, kh].contiguous().to(d), b2.to(d),
                                                        ln=(g.to(d), b.to(d)))
    _mlp_value_edges("mlp_block D %d" % D, D, H, M, run)


@pytest.mark.parametrize("D,H,M", [(384, 768, 130), (192, 384, 70)])
def test_mlp_stream_block_value_edges(D, H, M):
    d = dev()
    kd, kh = packing.kperm32(D), packing.kperm32(H)
    run = lambda x, g, b, w1, b1, w2, b2: ops.mlp_stream_block(x.to(d), packing.pack_stream_pair(w1[:, kd], w2[:, kh]).to(d), b1.to(d), b2.to(d), H,
                                                               ln=(g.to(d), b.to(d)))
    _mlp_value_edges("mlp_stream_block D %d" % D, D, H, M, run)


# ---------------------------------------------------------------------------------------------------
# softmax
def to_head_major(qkv, nseq, S, heads):
    dh = qkv.shape[1] // 3 // heads
    return qkv.view(nseq, S, 3, heads, dh).permute(0, 3, 2, 1, 4).contiguous().view(-1)


def _softmax(what, run, dtype, S, heads=2, dh=24, nseq=2):
    ratios = {}
    for name, qkv in ve.softmax_cases(S, heads, dh, dtype, nseq):
        want = ve.attn_ref(qkv, nseq, S, heads)
        got = run(qkv, nseq, S, heads).double().cpu()
        err = float((got - want).abs().max()) if bool(torch.isfinite(got).all()) else float("inf")
        ratios[name] = err / ve.softmax_bar(qkv, heads, tol(dtype, 3))
    _report("%s S %d" % (what, S), dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", [1, 16, 100, 256])
def test_attention_value_edges(dtype, S):
    _softmax("attention", lambda qkv, nseq, S_, heads: ops.attention(qkv.to(dev()), nseq, S_, heads), dtype, S)


@pytest.mark.parametrize("S,pair", [(256, None), (256, 1), (1024, None), (1024, 2)])
def test_attention_head_major_value_edges(S, pair):
    """the head-major kernels (fp16, S in {64, 256, 1024}): the shape rule's own choice and the long-window pair forms ("attn.hm_pair" 1 / 2)"""
    with ops.tuning({} if pair is None else {"attn.hm_pair": pair}):
        _softmax("attention_head_major%s" % ("" if pair is None else " hm_pair %d" % pair),
                 lambda qkv, nseq, S_, heads: ops.attention_head_major(to_head_major(qkv, nseq, S_, heads).to(dev()), nseq, S_, heads),
                 torch.float16, S)


# ---------------------------------------------------------------------------------------------------
# the fused LViT front half and the whole window block (fp16): the offset rides on the embedding bias, so it reaches norm1 (and, through the
# residual stream, norm2) inside the kernels
def _stage_bar_ratio(what, got, exact, model_out):
    model = float((model_out - exact).abs().max())
    err = float((got.double().cpu() - exact).abs().max())
    print("%s: max-abs %.3e, rounding model %.3e, measured / model %.2f" % (what, err, model, err / model))
    return err / (FP16_STAGE_MARGIN * model) if bool(torch.isfinite(got).all()) else float("inf")


def test_embed_qkv_value_edges():
    dt, d = torch.float16, dev()
    B, C, H, W, ws, p = 2, 24, 32, 32, 32, 2
    D, S = p * p * C, (ws // p) ** 2
    gen = torch.Generator().manual_seed(90)
    fmap = ops.to_nhwc(torch.randn(B, C, H, W, generator=gen).to(dt)).to(d)
    we, wq = (torch.randn(D, D, generator=gen) * D ** -0.5).to(dt), (torch.randn(3 * D, D, generator=gen) * D ** -0.5).to(dt)
    be, pos = 0.1 * torch.randn(D, generator=gen), torch.randn(S, D, generator=gen).to(dt)
    g, b = ln_operands(D)
    perm = packing.kperm32(D)
    tok = ops.patchify(fmap, C, ws, p).double().cpu()
    half = lambda t: t.to(dt).double()

    def block(bias, quant):                                  # cfen_oracle.vit_tokens up to the qkv projection, with its quant points
        x = quant(tok @ we.double().t() + bias.double() + tok + pos.double().repeat(tok.shape[0] // S, 1))
        return x, quant(cfen_oracle.layer_norm(x, g.double(), b.double()) @ wq.double().t())
    spread = float(block(be, lambda t: t)[0].std(-1).mean())
    ratios = {}
    for rho in (0, 8, 64):
        bias = be + rho * spread
        x1, qkv = ops.embed_qkv(fmap, C, ws, p, we[:, perm].contiguous().to(d), bias.to(d), pos.to(d), g.to(d), b.to(d), wq[:, perm].contiguous().to(d))
        ex, mo = block(bias, lambda t: t), block(bias, half)
        ratios["rho%d x1" % rho] = _stage_bar_ratio("embed_qkv rho %d x1" % rho, x1, ex[0], mo[0])
        ratios["rho%d qkv" % rho] = _stage_bar_ratio("embed_qkv rho %d qkv" % rho, qkv, ex[1], mo[1])
    _report("embed_qkv", dt, ratios)


_LVIT = {}


def _lvit_operands():
    """one LViT level-1 instance (C = 24, D = 96, 4 heads) with the deterministic 'trained' weight distribution, rounded to fp16; built once"""
    if not _LVIT:
        from cfen_vit_dehazing_amd.config import NetConfig
        from cfen_vit_dehazing_amd.manifest import generate_state_dict
        cfg = NetConfig(24, 4, patch_size=32, load_size=256)
        g = cfg.vit("localvit_encoder_01")
        full = generate_state_dict(cfg, seed=3, with_dead=False)
        sd = {k: (v.to(torch.float16) if v.dtype.is_floating_point else v) for k, v in full.items() if k.startswith(g.name + ".")}
        gen = torch.Generator().manual_seed(91)
        _LVIT.update(g=g, sd=sd, x=torch.randn(1, 24, 32, 32, generator=gen).to(torch.float16))
    return _LVIT["g"], dict(_LVIT["sd"]), _LVIT["x"]


def _lvit_case(what, g, sd16, x):
    dt, d = torch.float16, dev()
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd16.items()}
    exact = cfen_oracle.lvit(dict(sd64), g.name, x.double(), g.heads, 32)
    model = cfen_oracle.lvit(dict(sd64), g.name, x.double(), g.heads, 32, quant=lambda t: t.to(dt).double())
    pk = packing.pack_vit(sd16, g, dt)
    pk.update(packing.pack_lvit_window(sd16, g, dt))
    pk = {k: v.to(d).contiguous() for k, v in pk.items()}
    got = ops.from_nhwc(ops.lvit_window(ops.to_nhwc(x).to(d), 24, 32, 2, pk, g.name, g.hidden), 24)
    return _stage_bar_ratio(what, got, exact, model)


def test_lvit_window_value_edges():
    g, sd, x = _lvit_operands()
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    taps = {}
    cfen_oracle.vit_tokens(sd64, g.name, cfen_oracle.unfold_tokens(cfen_oracle.window_partition(x.double(), 32), 2), g.heads, taps=taps)
    spread = float(taps["embed"].std(-1).mean())
    ratios = {}
    for rho in (0, 8, 64):
        sdr = dict(sd)
        sdr[g.name + ".linear_encoding.bias"] = (sd[g.name + ".linear_encoding.bias"].double() + rho * spread).to(torch.float16)
        ratios["rho%d" % rho] = _lvit_case("lvit_window rho %d" % rho, g, sdr, x)
    _report("lvit_window", torch.float16, ratios)


def test_lvit_window_softmax_value_edges():
    """the window kernel's own softmax: the q rows of in_proj_weight times 8 make its scores 8 times as spread (a few keys carry a query's weight)"""
    g, sd, x = _lvit_operands()
    k = g.name + ".encoder.layers.0.self_attn.in_proj_weight"
    w = sd[k].clone()
    w[:g.dim] = (w[:g.dim].double() * 8).to(torch.float16)
    sd[k] = w
    _report("lvit_window softmax", torch.float16, {"q_x8": _lvit_case("lvit_window q x 8", g, sd, x)})


# ---------------------------------------------------------------------------------------------------
# ActNorm2d first-call initialisation on the device, from raw layer outputs at a mean of 64 spreads
ACTNORM_RAISED = ("sk_conv_d03r", "lgcat_conv_e01")        # a 1x1 conv on a concatenation early in decoder R, and the first level's fuse conv


def _oracle_actnorm_inputs(sd, x, cfg, monkeypatch):
    """float64 oracle forward of an uninitialised net -> {ActNorm prefix: the raw map its first call sees}"""
    rec = {}
    plain = cfen_oracle.actnorm

    def spy(sd_, prefix, t):
        if int(sd_[prefix + ".initialized"]) != 1:
            rec[prefix] = t
        return plain(sd_, prefix, t)
    monkeypatch.setattr(cfen_oracle, "actnorm", spy)
    cfen_oracle.forward({k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}, x.double(), cfg.num_heads, cfg.patch_size)
    monkeypatch.setattr(cfen_oracle, "actnorm", plain)
    return rec


def test_actnorm_device_init_value_edges(monkeypatch):
    """the bias of two convolutions in front of ActNorm layers raised by 64 of their channels' spreads: the device's first forward must still find
    -mean and -0.5 log(var) of those maps (cfen_oracle.actnorm_init_params in float64 on the oracle's own maps) to 4 x the error of the fp32
    two-pass restatement of that formula"""
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    from cfen_vit_dehazing_amd.manifest import generate_state_dict, synthetic_input
    from helpers import load_net_fixture
    cfg, batch, _ = load_net_fixture("refinit_tiny_nf24_hdr4")
    sd = generate_state_dict(cfg, seed=0, mode="reference_init")
    x = synthetic_input(batch, cfg)
    first = _oracle_actnorm_inputs(sd, x, cfg, monkeypatch)
    for conv in ACTNORM_RAISED:
        t = first[conv + ".1"]
        spread = t.transpose(0, 1).reshape(t.shape[1], -1).std(1)
        sd[conv + ".0.bias"] = (sd[conv + ".0.bias"].double() + 64.0 * spread).float()
    maps = _oracle_actnorm_inputs(sd, x, cfg, monkeypatch)
    net = dec_ipt(cfg, compute_dtype="fp32")
    net.load_state_dict(sd, strict=True)
    net = net.to("cuda:0")
    outs = net(x.to("cuda:0"))
    assert all(bool(torch.isfinite(o).all()) for o in outs)
    got = net.state_dict()
    ratios = {}
    for conv in ACTNORM_RAISED:
        t = maps[conv + ".1"]
        xt = t.transpose(0, 1).reshape(t.shape[1], -1)
        rho = float((xt.mean(1).abs() / xt.std(1)).min())
        assert 60.0 <= rho <= 70.0, (conv, rho)
        w64, b64 = cfen_oracle.actnorm_init_params(t)
        w32, b32 = ve.actnorm_init(t.float(), torch.float32)
        bar_w, bar_b = ve.BAR_FACTOR * float((w32.double() - w64).abs().max()), ve.BAR_FACTOR * float((b32.double() - b64).abs().max())
        dw = float((got[conv + ".1.weight"].double().cpu().flatten() - w64).abs().max())
        db = float((got[conv + ".1.bias"].double().cpu().flatten() - b64).abs().max())
        print("actnorm init %s (rho %.1f): weight error %.3e, bar %.3e; bias error %.3e, bar %.3e" % (conv, rho, dw, bar_w, db, bar_b))
        ratios[conv + " weight"], ratios[conv + " bias"] = dw / bar_w, db / bar_b
    _report("actnorm init", torch.float32, ratios)


# ---------------------------------------------------------------------------------------------------
# the padded token rows of the v5 LViT blocks (include/cfen_padnorm.h): the same cases over the real slots of a row, yardstick in padnorm_ref.py
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs,C", [(8, 6), (16, 12)])
def test_layernorm_padded_value_edges(dtype, cs, C):
    """every case over the real slots of rows of 4 pixels of cs slots.  fp32, measured on an MI355X (error / bar):
                               rho0   rho1   rho8    rho64    rho256   tiny_std  constant  alt_sign
      (8, 6)   correction      0.336  0.288  0.0853  5.42     19.6     5.55      0         5.42      (zero slots centred to -p, taken back out of the sums)
      (8, 6)   as shipped      0.311  0.288  0.0688  0.00777  0.00244  0.00675   0         0.00777   (a padding slot is 0 after centring, no correction)
      (16, 12) correction      0.282  0.199  0.0698  0.078    19.5     5.96      0         0.0487
      (16, 12) as shipped      0.276  0.163  0.0565  0.00951  0.00253  0.00745   0         0.0105
    fp16 with the correction formula: rho256 1.48 / 4.57, everything else under 1 (DESIGN 21 has the whole table)."""
    import padnorm_ref as pr
    d = dev()
    ratios = {}
    for case in ve.CASES:
        x, g, b, want, e32 = pr.yardstick(case, 33, cs, C, dtype)
        ratios[case] = ve.ratio(ops.layernorm(x.to(d), g.to(d), b.to(d), padded=(cs, C)), want, e32, dtype)
    assert set(ratios) == set(ve.CASES)
    _report("layernorm padded (cs %d, C %d)" % (cs, C), dtype, ratios)
