"""Without a GPU: tests/conv_rules.py against csrc/k_conv.hip, and the ledger of k_conv instantiations.

Every launch_conv_t<T, ...> / launch_conv_wl_t<T, ...> that launch_conv can return is parsed out of the source.  That set must equal the union of
  * the claims of the case tables of tests/test_hip_conv_geometry.py (each checked through conv_rules, in the dtype it is made for),
  * COVERED_ELSEWHERE: an existing operator test and the shape at which it reaches the instantiation (checked through conv_rules as well),
  * NOT_COVERED: a reason.
A new arm in the switch fails here until someone tests or excuses it; so does a case taken out of the tables."""
import os
import re

import pytest
import torch

import conv_rules as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_CONV = os.path.join(ROOT, "cfen_vit_dehazing_amd", "csrc", "k_conv.hip")
F16, F32 = "float16", "float32"

_UP = ("reachable through the generator only (ConvDesc::up4 has no operator entry point): tests/test_hip_net.py::"
       "test_gvit_upsampling_inside_the_fuse_conv_equals_the_upsample_launch runs the x4-source forms against the separate upsample launch")
NOT_COVERED = {
    ("wl_up", 2, 2, 8): _UP, ("wl_up", 2, 1, 4): _UP, ("wl_up", 2, 2, 4): _UP, ("wl_up", 3, 2, 8): _UP, ("wl_up", 3, 1, 4): _UP,
    ("wl_up", 3, 2, 4): _UP, ("wl_up", 4, 1, 8): _UP, ("wl_up", 6, 1, 8): _UP,
}

# instantiation -> (module, test, dtype, conv_rules.conv_problem arguments of the parametrisation that reaches it); all at batch 2
COVERED_ELSEWHERE = {
    ("plain", 1, 2): ("test_hip_ops", "test_conv_plain", F16, dict(B=2, Hout=32, Wout=32, cin=3, cout=12, k=5)),
    ("plain", 2, 1): ("test_hip_bounds", "test_conv_gather", F16, dict(B=2, Hout=32, Wout=32, cin=12, cout=24, k=3, wlds=0)),
    ("plain", 6, 1): ("test_hip_ops", "test_conv_gather_with_and_without_lds_staged_weights_is_bitwise_equal", F16,
                      dict(B=2, Hout=16, Wout=16, cin=48, cout=96, k=3, wlds=0)),
    ("plain", 8, 1): ("test_hip_ops", "test_conv_off_nf24_widths", F16, dict(B=2, Hout=16, Wout=16, cin=64, cout=128, k=3)),
    ("wl", 2, 1, 4): ("test_hip_ops", "test_conv_plain", F16, dict(B=2, Hout=32, Wout=32, cin=12, cout=24, k=3)),
    ("wl", 2, 2, 8): ("test_hip_ops", "test_conv_plain", F32, dict(B=2, Hout=32, Wout=32, cin=12, cout=24, k=3)),
    ("wl", 3, 1, 4): ("test_hip_ops", "test_conv_1x1_concat_actnorm_relu_residual", F16, dict(B=2, Hout=16, Wout=16, cin=48, cout=48, k=1, nsrc=2)),
    ("wl", 3, 2, 8): ("test_hip_ops", "test_conv_plain", F16, dict(B=2, Hout=16, Wout=16, cin=24, cout=48, k=3)),
    ("wl", 4, 1, 8): ("test_hip_ops", "test_conv_off_nf24_widths", F16, dict(B=2, Hout=16, Wout=16, cin=32, cout=64, k=3)),
    ("wl", 6, 1, 8): ("test_hip_ops", "test_conv_plain", F16, dict(B=2, Hout=16, Wout=16, cin=48, cout=96, k=3)),
}


def _source():
    with open(K_CONV) as f:
        return f.read()


def _launch_conv_body(src):
    start = src.index("int launch_conv(int ng, const ConvDesc* dp, hipStream_t s) {")
    return src[start:src.index("\n}\n", start)]


def instantiations_in_source():
    found = set()
    for wl, args in re.findall(r"launch_conv(_wl)?_t<T,\s*([^>]*)>", _launch_conv_body(_source())):
        a = [v.strip() for v in args.split(",")]
        nums = tuple(int(v) for v in a if v not in ("true", "false"))
        if not wl:
            assert len(a) == 2, args
            found.add(("plain",) + nums)
        else:
            assert len(nums) == 3 and len(a) in (3, 4), args
            found.add(("wl_up" if a[-1] == "true" else "wl",) + nums)
    return found


def _claims():
    """{instantiation: [case id]} over the GPU file's tables, each claim checked through conv_rules"""
    import test_hip_conv_geometry as tg
    claims = {}
    for c in tg.SIZE_CASES:
        for dtype in tg.DTYPES:
            assert tg.size_case_rule(c, dtype) == c.claim, "%s in %s" % (c.id, dtype)
        claims.setdefault(c.claim, []).append(c.id)
    for c in tg.GEOM_CASES:
        assert set(c.claim) == {F16, F32}, c.id
        for dtype in tg.DTYPES:
            inst = c.claim[str(dtype).replace("torch.", "")]
            assert tg.geom_case_rule(c, dtype) == inst, "%s in %s" % (c.id, dtype)
            claims.setdefault(inst, []).append(c.id)
    return claims


def test_the_parser_finds_the_switch():
    found = instantiations_in_source()
    assert len(found) >= 27, sorted(found)
    assert {("plain", 3, 4), ("wl", 2, 2, 4), ("wl_up", 6, 1, 8)} <= found


def test_every_instantiation_in_launch_conv_is_tested_or_excused():
    found = instantiations_in_source()
    claims = _claims()
    for inst, (module, test, dtype, kw) in COVERED_ELSEWHERE.items():
        assert cr.conv_problem(dtype, **kw) == inst, "%s::%s does not reach %r in %s at %r" % (module, test, inst, dtype, kw)
        assert callable(getattr(__import__(module), test)), "%s::%s is gone" % (module, test)
    ledger = set(claims) | set(COVERED_ELSEWHERE) | set(NOT_COVERED)
    assert found - ledger == set(), "instantiations in launch_conv that nothing tests or excuses: %r" % sorted(found - ledger)
    assert ledger - found == set(), "the ledger names instantiations launch_conv does not have: %r" % sorted(ledger - found)
    assert not set(NOT_COVERED) & (set(claims) | set(COVERED_ELSEWHERE)), "excused and tested at once"
    assert all(isinstance(r, str) and len(r) > 20 for r in NOT_COVERED.values())


def test_the_issue_list_of_unreached_instantiations_is_claimed_by_the_size_cases():
    import test_hip_conv_geometry as tg
    claimed = {c.claim for c in tg.SIZE_CASES}
    assert claimed == {("plain", 2, 2), ("plain", 3, 2), ("plain", 3, 4), ("plain", 4, 2), ("plain", 6, 2), ("wl", 2, 2, 4), ("wl", 3, 2, 4),
                       ("plain", 3, 1), ("plain", 4, 1)}
    assert not claimed & set(COVERED_ELSEWHERE)
    by_map = {}
    for c in tg.SIZE_CASES:
        by_map.setdefault(c.map, []).append(c)
        B, H, W = tg.MAPS[c.map]
        assert H % 2 == 1 and H != W and W % 16 == 0 and W % 64 != 0
        if c.claim[0] == "wl":                                  # the staged matrix stays below the 8-wave threshold in both dtypes
            assert c.wlds == cr.WLDS_SHIPPED
            for dtype in (F16, F32):
                assert cr.wl_bytes(dtype, cr.round_up(c.cout, 16), cr.kpad(dtype, cr.round_up(c.cin, 8), c.k, c.nsrc)) < cr.FAT_BYTES
        else:
            assert c.wlds == 0
    assert cr.shrink_of(3 * 187 * 480) == 1 and (3 * 187 * 480) % 256 != 0
    assert cr.shrink_of(5 * 211 * 1008) == 0 and (5 * 211 * 1008) % 64 == 16
    for m in ("px2e18", "px2e20"):                              # per map: an epilogue with a residual, and a stride-2 case from an odd input
        assert any(c.epi != "bias" for c in by_map[m]) and any(c.stride == 2 for c in by_map[m])


def test_small_geometry_cases_reach_every_instantiation_of_the_shipped_knobs_on_a_small_map():
    """at the shipped knobs ("conv.wlds" 2, every pixel count staged) a map below 2^18 pixels reaches these and no other"""
    import test_hip_conv_geometry as tg
    reach = set()
    for dtype in (F16, F32):
        for cout_pad in (16, 32, 48, 64, 96, 128):
            for Kpad in range(cr.kc(dtype), 2049, cr.kc(dtype)):
                reach.add(cr.launch_conv(dtype, 1, 3, 7, 48, 1, cout_pad, Kpad))
    reach = {i for i in reach if i[0] == "wl" or i[1] in (1, 8)}    # plain <2..6, 1>: matrices above 150 KB only, test_hip_ops.py has fp32 48 -> 96
    got = {c.claim[d] for c in tg.GEOM_CASES for d in (F16, F32)}
    assert got == reach, (sorted(got), sorted(reach))
    for c in tg.GEOM_CASES:
        Ho, Wo = tg.geom_out_hw(c)
        assert Ho != Wo and (c.Win if c.kind == "convT" else Wo) % 16 == 0


def test_restated_constants_are_the_ones_in_the_source():
    src = _source()
    body = _launch_conv_body(src)
    assert "px >= (1 << 20) ? 0 : px >= (1 << 18) ? 1 : 2" in body and (cr.SHRINK0_PX, cr.SHRINK1_PX) == (1 << 20, 1 << 18)
    assert body.count("wbytes >= 16 * 1024") == 2 and cr.FAT_BYTES == 16 * 1024
    assert "wbytes <= (wlm > 1 ? 150 : 60) * 1024 && px < (1ll << cfen_tune_conv_wlds_maxlog())" in body and cr.WLDS_KB == {1: 60, 2: 150}
    assert "(long long)ng * d.B * d.Hb * d.Wb * d.nphase" in body
    assert "return row + (m <= 32 ? 32 - m : 96 - m);" in src and "m = row & 63" in src
    assert "constexpr int ST_CHUNKS = 64;" in src and cr.ST_CHUNKS == 64
    assert "constexpr int U = 4;\n    for (int pb = p0 + my_p; pb < p1; pb += U * lanes_per_cv)" in src and cr.STATS_U == 4
    assert "const int per = (HW + ST_CHUNKS - 1) / ST_CHUNKS;" in src and "const int lanes_per_cv = 256 / cv;" in src
    assert "long long g = (nvec + 2047) / 2048;" in src and "(g > 128 ? 128 : g)" in src and (cr.GRID_IMG_VECS, cr.GRID_IMG_CAP) == (2048, 128)
    knobs = open(os.path.join(os.path.dirname(K_CONV), "cfen_tune_knobs.hpp")).read()
    assert 'CFEN_KNOB(conv_wlds, "conv.wlds", %d,' % cr.WLDS_SHIPPED in knobs
    assert 'CFEN_KNOB(conv_wlds_maxlog, "conv.wlds_maxlog", %d,' % cr.WLDS_MAXLOG_SHIPPED in knobs


def test_conv_rules_known_answers():
    assert [cr.conv_wl_pitch(F16, k) for k in (32, 64, 96, 160, 224)] == [96, 160, 224, 352, 480]
    assert [cr.conv_wl_pitch(F32, k) for k in (16, 48, 80, 144)] == [96, 224, 352, 608]
    assert all(cr.conv_wl_pitch(d, k) % 64 == 32 and 0 <= cr.conv_wl_pitch(d, k) - k * cr.esize(d) < 64
               for d in (F16, F32) for k in range(cr.kc(d), 1025, cr.kc(d)))
    assert cr.conv_wl_pitch(torch.float16, 96) == 224 and cr.kpad(torch.float32, 8, 3) == 80 and cr.kpad(F16, 8, 3) == 96
    # the rule's corners: a pixel count on either side of each threshold, the two "conv.wlds" sizes, "conv.wlds_maxlog"
    assert cr.launch_conv(F16, 1, 1, 1 << 9, (1 << 9), 1, 48, 96, wlds=0) == ("plain", 3, 2)
    assert cr.launch_conv(F16, 1, 1, 1 << 9, (1 << 9) - 16, 1, 48, 96, wlds=0) == ("plain", 3, 1)
    assert cr.launch_conv(F16, 1, 4, 1 << 9, (1 << 9), 1, 48, 96, wlds=0) == ("plain", 3, 4)
    assert cr.launch_conv(F16, 4, 1, 1 << 8, (1 << 8), 4, 48, 96, wlds=0) == ("plain", 3, 4)           # groups and phases count as pixels
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 96, 1024, wlds=1) == ("plain", 6, 1)                       # 96 x 2080 B > 60 KB
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 96, 1024, wlds=2) == ("plain", 6, 1)                       # ... > 150 KB too
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 96, 512, wlds=1) == ("plain", 6, 1)                        # 96 x 1056 B = 99 KB
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 96, 512, wlds=2) == ("wl", 6, 1, 8)
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 32, 96, wlds_maxlog=10) == ("wl", 2, 1, 4)             # 512 pixels < 2^10
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 32, 96, wlds_maxlog=9) == ("plain", 2, 1)
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 16, 96) == ("plain", 1, 2) and cr.launch_conv(F32, 1, 2, 16, 16, 1, 128, 96) == ("plain", 8, 1)
    assert cr.launch_conv(F16, 1, 2, 16, 16, 1, 48, 96, up4=True) == ("wl_up", 3, 1, 4)
    for bad in (dict(Cout_pad=80), dict(Cout_pad=112), dict(Cout_pad=144)):
        with pytest.raises(ValueError):
            cr.launch_conv(F16, 1, 2, 16, 16, 1, Kpad=96, **bad)
    with pytest.raises(ValueError):
        cr.launch_conv(F32, 1, 2, 16, 16, 1, 48, 96, up4=True)


def test_statistics_cases_have_the_chunks_they_are_there_for():
    import test_hip_conv_geometry as tg
    for c in tg.STATS_CASES:
        for d in c.dtypes:
            tg._check_stats_plan(c, getattr(torch, d))
    plans = {(c.id, d): tg.stats_case_facts(c, d) for c in tg.STATS_CASES for d in c.dtypes}
    assert any(p["empty"] > 0 for p in plans.values())                                        # chunks with no pixel
    assert any(p["passes"] > 1 and p["last_pixels"] < p["per"] for p in plans.values())      # several passes, a short last chunk
    assert any(p["passes"] > 1 and p["ragged"] < p["pass_pixels"] and p["idle"] > 0 for p in plans.values())   # 256 / cv not whole, ragged last pass
    assert sum(p["grid"] == cr.GRID_IMG_CAP for p in plans.values()) >= 2 and any(2 < p["grid"] < cr.GRID_IMG_CAP for p in plans.values())
    # what the operator tests had before: every chunk full and done in one partial pass, the apply grid far from its cap
    for C, HW in ((24, 1024), (96, 256), (128, 256), (24, 4096), (8, 4096)):
        for d in (F16, F32):
            p = cr.chan_stats_plan(d, HW, C)
            assert p["passes"] == 1 and p["ragged"] < p["pass_pixels"] and p["empty"] == 0 and p["last_pixels"] == p["per"]
            assert cr.grid_img(d, HW, C) <= 12
