"""CPU checks of include/cfen_padnorm.h: the header's ledger, argument errors that launch nothing, and the yardstick of padded rows
(padnorm_ref.py) -- the two-pass restatement stays inside its own bar, the fp32 restatement of the correction formula k_layernorm used for padded
rows does NOT (so the GPU test can see that defect), the restatement of the masked formula it uses now does, in every case."""
import ctypes

import pytest
import torch

import cabi_ledger
import padnorm_ref as pr
import value_edges_ref as ve

DTYPES = [torch.float32, torch.float16]
M = 200                                           # seeded rows per case
FNS = {"cfen_layernorm_padded": 11}


def test_padnorm_header_is_bound_and_guard_band_tested():
    cabi_ledger.check_header_bound("cfen_padnorm.h", FNS)
    cabi_ledger.check_guard_band_test_calls("test_hip_bounds.py", "test_guard_bands_padnorm", FNS)


def test_padnorm_argument_errors_do_not_need_a_gpu():
    """refused before any launch (the pointers are never followed): C > cs, C < 1, cs < 1, D no whole number of pixels, and what cfen_layernorm refuses"""
    lib = cabi_ledger.library().load()
    p = ctypes.c_void_p(1 << 20)

    def refused(what, dtype, M_, D, cs, C, x=p, y=p, g=p, b=p):
        assert lib.cfen_layernorm_padded(dtype, x, y, g, b, M_, D, cs, C, 1e-5, None) == -1, what
        err = lib.cfen_last_error()
        assert b"layernorm" in err and what in err, err
    refused(b"8 real slots per pixel of 6", 0, 5, 24, 6, 8)
    refused(b"0 real slots per pixel of 8", 0, 5, 32, 8, 0)
    refused(b"0 slots per pixel", 0, 5, 32, 0, 0)
    refused(b"-8 slots per pixel", 0, 5, 32, -8, 6)
    refused(b"rows of 40 slots are no whole number of pixels of 16", 1, 5, 40, 16, 12)
    refused(b"empty problem", 0, 0, 32, 8, 6)
    refused(b"D=36 unsupported", 1, 5, 36, 12, 6)              # a whole number of pixels, but no multiple of the 8-element fp16 vector
    refused(b"D=2064 unsupported", 0, 5, 2064, 8, 6)
    refused(b"unknown dtype", 2, 5, 32, 8, 6)
    refused(b"non-null and 16-byte aligned", 0, 5, 32, 8, 6, x=ctypes.c_void_p((1 << 20) + 4))
    refused(b"non-null and 16-byte aligned", 0, 5, 32, 8, 6, y=None)
    refused(b"gamma/beta required", 0, 5, 32, 8, 6, g=None)


def test_layouts_are_the_padded_v5_levels():
    from cfen_vit_dehazing_amd import packing
    assert [(packing.cs_of(C), C) for C in (6, 12)] == list(pr.LAYOUTS) and packing.cs_of(24) == 24
    for cs, C in pr.LAYOUTS:
        D, Dn = pr.dims(cs, C)
        m = pr.real_slots(cs, C)
        assert int(m.sum()) == Dn and bool(m[0]) and m.shape == (D,)
        x = pr.rows("rho8", 3, cs, C, torch.float32)
        assert bool((x[:, ~m] == 0).all()) and torch.equal(x[:, m], ve.rows("rho8", 3, Dn, torch.float32))
        g, b = pr.ln_operands(cs, C)
        assert bool((g[~m] == 0).all()) and bool((b[~m] == 0).all()) and bool((g[m] != 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs,C", pr.LAYOUTS)
def test_two_pass_restatement_is_inside_its_own_bar(dtype, cs, C):
    for case in ve.CASES:
        x, g, b, want, e32 = pr.yardstick(case, M, cs, C, dtype)
        r32 = pr.layernorm(x, g, b, cs, C, torch.float32)
        assert bool(torch.isfinite(r32).all()), case
        assert ve.ratio(r32.to(dtype), want, e32, dtype) <= 1.0, case
        assert bool((want[:, ~pr.real_slots(cs, C)] == 0).all())


def _ratios(formula, dtype, cs, C, out_dtype=None):
    out = {}
    for case in ve.CASES:
        x, g, b, want, e32 = pr.yardstick(case, M, cs, C, dtype)
        got = pr.kernel_restated(x, g, b, cs, C, formula)
        out[case] = ve.ratio(got.to(out_dtype or dtype), want, e32, out_dtype or dtype)
    assert set(out) == set(ve.CASES)              # the share of cases left out is zero
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs,C", pr.LAYOUTS)
def test_the_correction_formula_misses_the_bar(dtype, cs, C):
    """the defect the GPU test is for is visible to it: taking (D - Dn) (p + mean)^2 back out of an fp32 sum of squares leaves nothing of a variance
    that is 64^-2 .. 256^-2 of it.  The statistics are fp32 for either storage type; the bar of the fp32 OUTPUT is asserted for both (an fp16 output's
    2^-10 |want| hides a relative error of the inverse deviation below 1e-3, which is what rho64 and tiny_std have: those ratios are printed)"""
    r = _ratios("correction", dtype, cs, C, out_dtype=torch.float32)
    print("correction formula, %s rows, (cs %d, C %d), fp32 output: error / bar  %s" % (dtype, cs, C, "  ".join("%s %.3g" % kv for kv in r.items())))
    for case in ("rho64", "rho256", "tiny_std"):
        assert r[case] > 1.0, (case, r)
    for case in ("rho0", "rho1"):
        assert r[case] <= 1.0, (case, r)
    if dtype == torch.float16:
        r16 = _ratios("correction", dtype, cs, C)
        print("correction formula, fp16 output: error / bar  %s" % "  ".join("%s %.3g" % kv for kv in r16.items()))
        assert r16["rho256"] > 1.0, r16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cs,C", pr.LAYOUTS)
def test_the_masked_formula_holds_the_bar_in_every_case(dtype, cs, C):
    r = _ratios("masked", dtype, cs, C)
    r.update({k + " (fp32 out)": v for k, v in _ratios("masked", dtype, cs, C, out_dtype=torch.float32).items()})
    print("masked formula, %s, (cs %d, C %d): error / bar  %s" % (dtype, cs, C, "  ".join("%s %.3g" % kv for kv in r.items())))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad
    x, g, b, _, _ = pr.yardstick("rho256", M, cs, C, dtype)
    assert bool((pr.kernel_restated(x, g, b, cs, C, "masked")[:, ~pr.real_slots(cs, C)] == 0).all())


@pytest.mark.parametrize("cs,C", pr.LAYOUTS)
def test_the_masked_formula_is_the_unpadded_kernel_on_the_real_slots(cs, C):
    """nothing of a padding slot enters: with garbage in the padding slots of x the masked restatement gives the same real outputs"""
    x, g, b, _, _ = pr.yardstick("rho64", 16, cs, C, torch.float32)
    m = pr.real_slots(cs, C)
    dirty = x.clone()
    dirty[:, ~m] = 1e30
    assert torch.equal(pr.kernel_restated(dirty, g, b, cs, C, "masked"), pr.kernel_restated(x, g, b, cs, C, "masked"))
