#!/usr/bin/env python3
"""What error should a CORRECT fp16 forward have at each of the 58 stages?  Writes tests/golden/fp16_stage_model.json.  CPU only.

The model is the float64 oracle (oracle/cfen_oracle.py) run the way the unfused fp16 plan runs: weights and input rounded to fp16 and
every tensor that plan stores rounded to fp16 (`quant`, see the oracle's docstring), all sums exact.  Its distance from the float64 oracle
on the unrounded weights is recorded per fixture and stage:
    rms          rms of the exact stage
    rel_rms      rms(model - exact) / rms over the whole tensor
    rel_rms_smp  the same at the fixture's 512 sample positions (helpers.sample_idx; what the full-size fixtures hold of the reference)
    max_abs_smp  max |model - exact| at those positions
    max_abs      max |model - exact| over the whole tensor (what a whole-tensor test compares its own whole-tensor maximum with)
tests/test_hip_net_fp16_stages.py holds the GPU's fp16 plan to a small multiple of these numbers; tests/test_fp16_stage_model_host.py
shows that wiring mistakes inside a transformer block land above that multiple.

Fixtures named refinit_* take the ActNorm parameters the fixture recorded (the reference's first forward), as the fp16 tests of those do.

Usage: gen_fp16_stage_model.py [fixture ...]      (no argument: every fixture of FIXTURES, and the JSON is rewritten)
"""
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import numpy as np
import torch

import cfen_oracle
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.manifest import generate_state_dict, synthetic_input

GOLDEN = os.path.join(ROOT, "tests", "golden")
JSON_PATH = os.path.join(GOLDEN, "fp16_stage_model.json")
OUTPUTS = ("tail_R", "tail_S", "tail_D")

OFF_NF24 = ["tiny_nf32_hdr6", "tiny_nf16_hdr3", "tiny_nf8_hdr4", "tiny_nf32_hdr6_h8"]
TINY = ["tiny_nf24_hdr4", "tiny_nf24_hdr2", "small_nf24_hdr4"] + OFF_NF24 + ["cfs_tiny_nf24_hdr4", "crs_tiny_nf24_hdr4", "v5_tiny_nf24_hdr4",
                                                                             "refinit_tiny_nf24_hdr4"]
FULL = ["full512_nf24_hdr4", "full512_nf32_hdr6", "full512b2_nf24_hdr4", "full512_nf24_hdr2", "full1024_nf24_hdr4"]
FIXTURES = TINY + FULL


def quant_fp16(t):
    return t.half().double()


def _variant(name):
    base = name[len("refinit_"):] if name.startswith("refinit_") else name
    for v in ("cfs", "crs", "v5"):
        if base.startswith(v + "_"):
            return v
    return "v3"


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, "net_%s.npz" % name))
    nf, hdr, ps, ls = [int(v) for v in z["cfg"]]
    heads = int(z["num_heads"]) if "num_heads" in z else 4
    return NetConfig(nf, hdr, patch_size=ps, load_size=ls, num_heads=heads, variant=_variant(name)), int(z["batch"]), z


def sample_idx(name, numel, n=512):
    """the sample positions of tools/gen_golden.py (tests/helpers.sample_idx)"""
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return torch.randint(0, numel, (n,), generator=g)


def fixture_weights_and_input(name):
    """(cfg, float64 state dict, float64 input, stage names) of a fixture; refinit_*: with the fixture's ActNorm parameters loaded"""
    cfg, batch, z = load_fixture(name)
    sd = generate_state_dict(cfg, seed=0, with_dead=False, mode="reference_init" if name.startswith("refinit") else "trained")
    if "actnorm_names" in z:
        for k in [str(v) for v in z["actnorm_names"]]:
            sd[k + ".weight"], sd[k + ".bias"] = torch.from_numpy(z["actnorm_w/" + k]), torch.from_numpy(z["actnorm_b/" + k])
            sd[k + ".initialized"] = torch.tensor(1)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return cfg, sd, synthetic_input(batch, cfg).double(), [str(s) for s in z["stage_names"]]


def rounded(sd):
    """the state dict as the fp16 net holds it"""
    return {k: (quant_fp16(v) if v.is_floating_point() else v) for k, v in sd.items()}


def exact_and_model(cfg, sd, x):
    """(exact stages, model stages): dicts of float64 NCHW tensors, the three outputs under tail_R / tail_S / tail_D"""
    ex, mo = {}, {}
    with torch.no_grad():
        cfen_oracle.forward(dict(sd), x, cfg.num_heads, cfg.patch_size, stages=ex, variant=cfg.variant)
        cfen_oracle.forward(rounded(sd), quant_fp16(x), cfg.num_heads, cfg.patch_size, stages=mo, variant=cfg.variant, quant=quant_fp16)
    return ex, mo


def stage_entry(name, exact, model):
    d = (model - exact).flatten()
    e = exact.flatten()
    idx = sample_idx(name, e.numel())
    rms = float(e.pow(2).mean().sqrt())
    rms_smp = float(e[idx].pow(2).mean().sqrt())
    return {"rms": rms,
            "rel_rms": float(d.pow(2).mean().sqrt()) / rms,
            "rel_rms_smp": float(d[idx].pow(2).mean().sqrt()) / rms_smp,
            "max_abs_smp": float(d[idx].abs().max()),
            "max_abs": float(d.abs().max())}


def model_entry(name):
    cfg, sd, x, names = fixture_weights_and_input(name)
    ex, mo = exact_and_model(cfg, sd, x)
    return {n: stage_entry(n, ex[n], mo[n]) for n in names}


def main(argv):
    names = argv or FIXTURES
    table = {}
    if argv and os.path.exists(JSON_PATH):
        with open(JSON_PATH) as f:
            table = json.load(f)
    t_all = time.time()
    for name in names:
        t0 = time.time()
        table[name] = model_entry(name)
        rel = [v["rel_rms"] for v in table[name].values()]
        print("%-26s %2d stages  rel rms %.2e .. %.2e  (%.1f s)" % (name, len(rel), min(rel), max(rel), time.time() - t0), flush=True)
    with open(JSON_PATH, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s in %.0f s" % (os.path.relpath(JSON_PATH, ROOT), time.time() - t_all))


if __name__ == "__main__":
    main(sys.argv[1:])
