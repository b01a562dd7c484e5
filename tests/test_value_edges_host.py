"""CPU checks of the value-edge yardstick (value_edges_ref.py): the fp32 two-pass restatements stay inside their own bar in every case, a one-pass
fp32 model of the statistics does not at rho = 256 (so the GPU tests can see the defect they are for), and the builders deliver the rho they claim."""
import pytest
import torch

import value_edges_ref as ve
from value_edges_ref import fold_operands, ln_operands

DTYPES = [torch.float32, torch.float16]
LN_SHAPES = [(5, 96), (33, 384), (7, 2048)]
FOLD_SHAPES = [(100, 384, 96), (33, 1536, 96), (33, 384, 768), (33, 256, 96), (128, 1536, 96), (16, 64, 128)]      # (M, K, N) of the gemm_ln / split-K / chain tests
IN_SHAPES = [(2, 24, 32, 32), (1, 8, 64, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,D", LN_SHAPES)
def test_layernorm_restatement_is_inside_its_own_bar(dtype, M, D):
    g, b = ln_operands(D)
    for case in ve.CASES:
        x = ve.rows(case, M, D, dtype)
        want = ve.layernorm(x, g, b, torch.float64)
        r32 = ve.layernorm(x, g, b, torch.float32)
        assert bool(torch.isfinite(r32).all()), case
        assert ve.ratio(r32.to(dtype), want, ve.e32_of(r32, want), dtype) <= 1.0, case


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", FOLD_SHAPES)
def test_folded_gemm_restatement_is_inside_its_own_bar(dtype, M, K, N):
    wl, s, bl = fold_operands(K, N, dtype)
    for case in ve.CASES:
        x = ve.rows(case, M, K, dtype)
        want = ve.gemm_ln(x, wl, s, bl, torch.float64)
        r32 = ve.gemm_ln(x, wl, s, bl, torch.float32)
        assert bool(torch.isfinite(r32).all()), case
        assert ve.ratio(r32.to(dtype), want, ve.e32_of(r32, want), dtype) <= 1.0, case


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,C,H,W", IN_SHAPES)
def test_instnorm_restatement_is_inside_its_own_bar(dtype, B, C, H, W):
    x, names = ve.channels(B, C, H, W, dtype)
    assert set(names) == set(ve.CASES)                      # no case left out
    want = ve.instnorm_relu(x, torch.float64)
    r32 = ve.instnorm_relu(x, torch.float32)
    for case in ve.CASES:
        ch = [c for c, n in enumerate(names) if n == case]
        e32 = ve.e32_of(r32[:, ch], want[:, ch])
        assert ve.ratio(r32[:, ch].to(dtype), want[:, ch], e32, dtype) <= 1.0, case


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_pass_fp32_statistics_violate_the_bar_at_rho_256(dtype):
    """the defect the GPU tests are for is visible to them: E[x^2] - mean^2 from fp32 sums, in the folded GEMM at K = 1536, the LayerNorm at
    D = 384 and the instance norm at 64 x 64, misses the bar at rho = 256 in both dtypes -- and stays inside it at rho = 1, where the present
    suite runs"""
    M, K, N = 33, 1536, 96
    wl, s, bl = fold_operands(K, N, dtype)
    g, b = ln_operands(384)
    for case, red in (("rho256", True), ("rho1", False)):
        x = ve.rows(case, M, K, dtype)
        want = ve.gemm_ln(x, wl, s, bl, torch.float64)
        e32 = ve.e32_of(ve.gemm_ln(x, wl, s, bl, torch.float32), want)
        one = ve.gemm_ln(x, wl, s, bl, torch.float32, stats=ve.stats_one_pass)
        r_fold = ve.ratio(one.to(dtype), want, e32, dtype)
        x = ve.rows(case, 33, 384, dtype)
        want = ve.layernorm(x, g, b, torch.float64)
        e32 = ve.e32_of(ve.layernorm(x, g, b, torch.float32), want)
        r_ln = ve.ratio(ve.layernorm(x, g, b, torch.float32, stats=ve.stats_one_pass).to(dtype), want, e32, dtype)
        ratios = [r_fold, r_ln]
        xc, names = ve.channels(1, 8, 64, 64, dtype)
        c = names.index(case)
        want = ve.instnorm_relu(xc[:, c:c + 1], torch.float64)
        e32 = ve.e32_of(ve.instnorm_relu(xc[:, c:c + 1], torch.float32), want)
        chan = lambda t, dim: ve.stats_one_pass(t, dim, finish=torch.float64)     # fp32 sums per chunk of 64 pixels, finished in double
        ratios.append(ve.ratio(ve.instnorm_relu(xc[:, c:c + 1], torch.float32, stats=chan).to(dtype), want, e32, dtype))
        print("one-pass fp32 model, %s, %s: error / bar = folded GEMM %.2f, LayerNorm %.2f, instance norm %.2f" % ((case, dtype) + tuple(ratios)))
        for r in ratios:
            assert (r > 1.0) if red else (r <= 1.0), (case, ratios)


@pytest.mark.parametrize("dtype", DTYPES)
def test_builders_deliver_the_claimed_rho(dtype):
    for M, D in LN_SHAPES + [(2, 1024), (1, 4096)]:
        for r in ve.RHOS:
            x = ve.rows("rho%d" % r, M, D, dtype)
            assert bool(torch.isfinite(x).all()) and float(x.abs().max()) <= 300.0
            got = ve.rho_of(x)
            # fp16 rounds values near 256 to multiples of 1/8 .. 1/4: the spread grows by under 1 % and the mean moves by under 0.01
            assert float((got - r).abs().max()) <= 0.01 * r + 0.02, (r, got)
        assert float((ve.rho_of(ve.rows("tiny_std", M, D, dtype)) - 100).abs().max()) <= (0.5 if dtype == torch.float32 else 5.0)
        c = ve.rows("constant", M, D, dtype)
        assert bool((c == c[:, :1]).all()) and bool((c.double() * 4 == (c.double() * 4).round()).all())
        a = ve.rows("alt_sign", M, D, dtype).double().mean(-1)
        assert bool(((a - ve.ALT_RHO * (1 - 2 * (torch.arange(M) % 2))).abs() <= 0.02).all())
    x, names = ve.channels(2, 24, 32, 32, dtype)
    flat = x.double().flatten(2)
    for c, n in enumerate(names):
        if n.startswith("rho"):
            assert float((ve.rho_of(flat[:, c]) - int(n[3:])).abs().max()) <= 0.01 * int(n[3:]) + 0.02
        elif n == "alt_sign":
            assert float(flat[0, c].mean()) > 60 and float(flat[1, c].mean()) < -60
        elif n == "constant":
            assert float(flat[:, c].max() - flat[:, c].min()) == 0.0


def test_softmax_cases_are_in_range_and_do_what_they_say():
    import math
    heads, dh = 2, 24
    for dtype in DTYPES:
        for S in (1, 16, 100, 256, 1024):
            cases = dict(ve.softmax_cases(S, heads, dh, dtype))
            assert {"ties", "offset1e3", "offset1e4", "negative", "dominant0", "dominant%d" % (S - 1)} <= set(cases)
            for nm, qkv in cases.items():
                assert bool(torch.isfinite(qkv).all()) and float(qkv.abs().max()) <= 320.0, nm
                q, k, v = qkv.double().view(2, S, 3, heads, dh).permute(2, 0, 3, 1, 4)
                sc = q @ k.transpose(-1, -2) / math.sqrt(dh)
                if nm == "ties":
                    want = v.mean(2, keepdim=True).expand_as(v).transpose(1, 2).reshape(2 * S, heads * dh)
                    assert float((ve.attn_ref(qkv, 2, S, heads) - want).abs().max()) <= 1e-12
                elif nm.startswith("offset"):
                    # about 1e3 / 1e4 in common (a query's own share of it varies with the query), O(1) between the keys of one query
                    assert 0.7 * float(nm[6:]) <= float(sc.mean()) <= 1.3 * float(nm[6:]) and float(sc.min()) >= 0.4 * float(nm[6:])
                    assert float((sc.amax(-1) - sc.amin(-1)).max()) <= 40.0
                elif nm == "negative":
                    assert float(sc.max()) <= -200.0
                elif S > 3:
                    p = int(nm[8:])
                    assert int(sc[:, :, 3].argmax(-1).unique()) == p
    assert ve.dominant_positions(100) == [0, 97, 99] and ve.dominant_positions(1024) == [0, 127, 128, 255, 256, 1023]
