"""The fp16 rounding model (oracle `quant`, tools/gen_fp16_stage_model.py, tests/golden/fp16_stage_model.json) on the host:
  * the committed numbers are what the tool computes today;
  * `quant=None` leaves the oracle what it was;
  * wiring mistakes inside a transformer block -- a wrong softmax scale, a dropped slice of the hidden layer, a dropped position row, heads
    paired with the wrong keys -- move that block's stage further than MARGIN x the model allows, i.e. tests/test_hip_net_fp16_stages.py
    would fail on a kernel that made them.

What the stage bar cannot see: single-element slips.  One dropped bias element moves its stage by 4e-5 .. 1e-3 relative rms, below fp16
rounding noise at whole-net depth; those stay the job of the operator tests (tests/test_hip_ops.py), which compare one kernel on its own
operands with float64."""
import importlib.util
import json
import os

import pytest
import torch

import cfen_oracle
from helpers import load_net_fixture, check_outputs, check_stages, FP16_STAGE_MARGIN as MARGIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("gen_fp16_stage_model", os.path.join(ROOT, "tools", "gen_fp16_stage_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


gen = _tool()


@pytest.fixture(scope="module")
def table():
    with open(gen.JSON_PATH) as f:
        return json.load(f)


def test_the_table_covers_every_fixture_and_stage(table):
    assert sorted(table) == sorted(gen.FIXTURES)
    for name in gen.FIXTURES:
        _, _, z = load_net_fixture(name)
        assert sorted(table[name]) == sorted(str(s) for s in z["stage_names"]), name
        for n, e in table[name].items():
            assert sorted(e) == ["max_abs", "max_abs_smp", "rel_rms", "rel_rms_smp", "rms"]
            # fp16 keeps 11 bits: one rounding is 2^-11 / sqrt(3) = 2.8e-4 relative rms at best, and nothing in a sane net sits 20 roundings deep in quadrature
            assert 1e-4 < e["rel_rms"] < 6e-3 and 1e-4 < e["rel_rms_smp"] < 6e-3 and 0 < e["max_abs_smp"] <= e["max_abs"], (name, n, e)


@pytest.mark.parametrize("name", ["tiny_nf24_hdr4", "tiny_nf24_hdr2", "tiny_nf8_hdr4", "cfs_tiny_nf24_hdr4", "v5_tiny_nf24_hdr4", "refinit_tiny_nf24_hdr4"])
def test_regenerating_reproduces_the_committed_numbers(table, name):
    """float64 sums of a fixed graph: the only freedom is the BLAS's summation order, ~1e-16 relative on the stage, which the subtraction of two
    forwards 1e-3 apart leaves at ~1e-12 of the recorded figure; a moved rounding point moves a figure by percents"""
    got = gen.model_entry(name)
    assert sorted(got) == sorted(table[name])
    for n, e in got.items():
        for k, v in e.items():
            assert abs(v - table[name][n][k]) <= 1e-6 * abs(table[name][n][k]), (name, n, k, v, table[name][n][k])


@pytest.mark.parametrize("name", ["tiny_nf24_hdr4", "crs_tiny_nf24_hdr4", "v5_tiny_nf24_hdr4"])
def test_quant_none_is_the_oracle_and_an_identity_quant_changes_nothing(name):
    """quant=None: the path test_oracle_golden.py pins (checked here against the same vectors at the same bars).  quant = identity walks every
    `quant` branch and must give the same bits -- except lgcat_conv_d01*, which that branch records as (stage + xf) - xf"""
    cfg, sd, x, names = gen.fixture_weights_and_input(name)
    _, _, z = load_net_fixture(name)
    sd32 = {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}
    st = {}
    with torch.no_grad():
        outs = cfen_oracle.forward(dict(sd32), x.float(), cfg.num_heads, cfg.patch_size, stages=st, variant=cfg.variant)
        also = cfen_oracle.forward(dict(sd32), x.float(), cfg.num_heads, cfg.patch_size, variant=cfg.variant, quant=None)
    check_outputs(z, outs, 5e-6)
    check_stages(z, st, 5e-5)
    assert all(torch.equal(a, b) for a, b in zip(outs, also))
    a, b = {}, {}
    with torch.no_grad():
        cfen_oracle.forward(dict(sd), x, cfg.num_heads, cfg.patch_size, stages=a, variant=cfg.variant)
        cfen_oracle.forward(dict(sd), x, cfg.num_heads, cfg.patch_size, stages=b, variant=cfg.variant, quant=lambda t: t)
    assert list(a) == list(b) == names
    for n in names:
        if n.startswith(("lgcat_conv_d01", "us_conv_d01", "tail_")):      # (stage + xf) summed in the other order, and what reads it
            assert float((a[n] - b[n]).abs().max()) <= 1e-13 * max(1.0, float(a[n].abs().max())), n
        else:
            assert torch.equal(a[n], b[n]), n


# ---- sensitivity: would the stage bar catch a wiring mistake inside a block? --------------------------------------------------------

SENS = "full512_nf24_hdr4"      # n_feats 24, hidden_dim_ratio 4, load size 256, patch 32: every GViT block has several tokens (level 3: 16), so the softmax mutants bite


def _block_inputs():
    """block name -> (kind, level, name of the stage it reads)"""
    blocks = {}
    for l in (1, 2, 3):
        src = "ds_conv_e0%d" % l
        blocks["localvit_encoder_0%d" % l] = ("l", l, src)
        blocks["globalvit_encoder_0%d" % l] = ("g", l, src)
    for t in "rsd":
        for l in (3, 2, 1):
            src = "lgcat_conv_e03" if l == 3 else ("cfsm2g_d0%dd" % (l + 1) if t == "d" else "sk_conv_d0%d%s" % (l + 1, t))
            blocks["localvit_decoder_0%d%s" % (l, t)] = ("l", l, src)
            blocks["globalvit_decoder_0%d%s" % (l, t)] = ("g", l, src)
    return blocks


def _mutants(sd, prefix, heads, S):
    """name -> {key: mutated tensor}; pure weight edits"""
    e = prefix + ".encoder.layers.0"
    w = sd[e + ".self_attn.in_proj_weight"]
    D = w.shape[1]
    dh = D // heads
    a = w.clone()
    a[:D] /= 1.155                                        # the softmax scale of a head width of 32 where 24 is meant: sqrt(32 / 24)
    b = sd[prefix + ".mlp_head.3.weight"].clone()
    b[:, -32:] = 0                                        # the last 32 hidden units never reach the output
    c = sd[prefix + ".position_encoding.pe.weight"].clone()
    c[S - 1] = 0                                          # the last token's position row
    d = w.clone()
    d[D + dh:D + 2 * dh], d[D + 2 * dh:D + 3 * dh] = w[D + 2 * dh:D + 3 * dh].clone(), w[D + dh:D + 2 * dh].clone()   # heads 1 and 2 read each other's keys
    return {"a: softmax scale / 1.155": {e + ".self_attn.in_proj_weight": a}, "b: last 32 hidden units of mlp_head dropped": {prefix + ".mlp_head.3.weight": b},
            "c: last position row dropped": {prefix + ".position_encoding.pe.weight": c}, "d: K of heads 1 and 2 swapped": {e + ".self_attn.in_proj_weight": d}}


def test_block_wiring_mutants_land_above_the_stage_bar(table):
    cfg, sd, x, _ = gen.fixture_weights_and_input(SENS)
    st = {}
    with torch.no_grad():
        cfen_oracle.forward(dict(sd), x, cfg.num_heads, cfg.patch_size, stages=st, variant=cfg.variant)
    blocks = _block_inputs()
    assert len(blocks) == 24
    worst = {}
    failed = []
    for name, (kind, l, src) in blocks.items():
        heads = cfg.num_heads << (l - 1)
        xin = st[src]

        def run(weights):
            with torch.no_grad():
                if kind == "l":
                    return cfen_oracle.lvit(weights, name, xin, heads, cfg.patch_size)
                return cfen_oracle.gvit(weights, name, xin, heads)
        base = run(sd)
        assert torch.equal(base, st[name]), name          # the block alone on its recorded input IS the stage
        S = (cfg.patch_size // 2) ** 2 if kind == "l" else (xin.shape[-1] // 16) ** 2
        assert S >= 4, name
        rms = float(base.pow(2).mean().sqrt())
        bar = MARGIN * table[SENS][name]["rel_rms"]
        for mname, edit in _mutants(sd, name, heads, S).items():
            w = dict(sd)
            w.update(edit)
            rel = float((run(w) - base).pow(2).mean().sqrt()) / rms
            ratio = rel / bar
            print("%-24s %-44s rel rms %.2e  bar %.2e  ratio %5.2f" % (name, mname, rel, bar, ratio))
            if mname not in worst or ratio < worst[mname][0]:
                worst[mname] = (ratio, name, rel, bar)
            if not rel > bar:
                failed.append((name, mname, rel, bar))
    for mname, (ratio, name, rel, bar) in worst.items():
        print("smallest separation of mutant %-44s %.2f at %s (rel rms %.2e against a bar of %.2e)" % (mname, ratio, name, rel, bar))
    assert not failed, "mutants the stage bar would let through (block, mutant, rel rms, bar): %r" % failed
