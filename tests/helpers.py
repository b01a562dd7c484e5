"""Shared helpers for the parity tests (fixture loading; no reference import: /root/reference does
not exist on the GPU box)."""
import os
import zlib

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd.config import NetConfig

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(autouse=True)
def knobs_at_shipped_defaults():
    """The tuning knobs are process-wide: a test that leaves one changed changes what every later test of the process runs.  Imported by the GPU
    test modules (autouse there): after every test, every knob must be at its shipped default again -- tests change knobs inside `with ops.tuning`.
    Offenders are put back before the assertion, so one slip fails one test."""
    yield
    from cfen_vit_dehazing_amd import ops
    left = ops.tune_not_shipped()
    for key, (_, shipped) in left.items():
        ops.tune(key, shipped)
    assert not left, "knobs left off their shipped default {key: (value, default)}: %r" % left


def load_net_fixture(name):
    z = np.load(os.path.join(GOLDEN, "net_%s.npz" % name))
    nf, hdr, ps, ls = [int(v) for v in z["cfg"]]
    heads = int(z["num_heads"]) if "num_heads" in z else 4        # the older fixtures were all made at the reference default of 4
    cfg = NetConfig(nf, hdr, patch_size=ps, load_size=ls, num_heads=heads, variant=variant_of(name))
    return cfg, int(z["batch"]), z


def variant_of(name):
    """fixture name -> generator variant (config.VARIANTS): [refinit_]{cfs,crs,v5}_* are the sibling generators, the rest is v3"""
    base = name[len("refinit_"):] if name.startswith("refinit_") else name
    for v in ("cfs", "crs", "v5"):
        if base.startswith(v + "_"):
            return v
    return "v3"


def weight_mode(name):
    """fixtures named refinit_* were made with the reference's own init distribution and uninitialised ActNorm (tools/gen_golden.py)"""
    return "reference_init" if name.startswith("refinit") else "trained"


def sample_idx(name, numel, n=512):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)
    return torch.randint(0, numel, (n,), generator=g)


def gpu_stages(net, z):
    """every stage but the tails of the v3 / v5 net's last forward, by fixture stage name"""
    st = {}
    xf = net.stage("ds_conv_e01")
    for n in [str(s) for s in z["stage_names"]]:
        if n.startswith("tail_"):
            continue
        t = net.stage(n)
        if n.startswith("lgcat_conv_d01"):
            t = t - xf                      # the plan folds `+ xf` (v3:696,852,1008) into this stage's epilogue
        st[n] = t
    return st


def _cfs_stages(net, z):
    """gpu_stages for the sibling generators (cfs / crs run level 1 on the head's own output)"""
    st = {}
    xf = net.stage("head" if net.cfg.full_res else "ds_conv_e01")
    for n in [str(s) for s in z["stage_names"]]:
        if n.startswith("tail_"):
            continue
        t = net.stage(n)
        if n.startswith("lgcat_conv_d01"):
            t = t - xf                      # `+ xf` (cfs:669,823,977) rides on this stage's epilogue
        st[n] = t
    return st


def check_stages(z, stages, tol, rel_sum=1e-4):
    """Compare a dict of stage tensors (NCHW, CPU) against the fixture's samples and checksums."""
    worst = 0.0
    for n in [str(s) for s in z["stage_names"]]:
        t = stages[n].float().cpu()
        assert tuple(t.shape) == tuple(int(v) for v in z["stage_shape/" + n]), n
        smp = t.flatten()[sample_idx(n, t.numel())].numpy()
        d = float(np.abs(smp - z["stage_smp/" + n]).max())
        worst = max(worst, d)
        assert d <= tol, "stage %s: sampled max-abs %.3e > %.1e" % (n, d, tol)
        ref_abs = float(z["stage_abs/" + n])
        got_abs = float(t.double().abs().sum())
        assert abs(got_abs - ref_abs) <= rel_sum * ref_abs + 1e-6, "stage %s abs-sum %.6f vs %.6f" % (n, got_abs, ref_abs)
    return worst


# ---- the fp16 stage bar (tools/gen_fp16_stage_model.py -> golden/fp16_stage_model.json) ----
# One number for every stage and fixture: the fp16 plan may sit this many times further from the exact result than the rounding model does.  3 = the kernels
# sum in another order than the model's exact sums (and in fp32, the model in float64), the fused kernels round at fewer points than the unfused plan the model
# follows, and a maximum over 512 samples scatters by tens of percent between two realisations of the same noise.  It is a bar on the model: a stage that exceeds
# it is a missing rounding point of the model or a kernel that loses accuracy, never a reason to raise it.
FP16_STAGE_MARGIN = 3.0


def fp16_stage_model():
    import json
    with open(os.path.join(GOLDEN, "fp16_stage_model.json")) as f:
        return json.load(f)


def check_outputs(z, outs, tol):
    worst = 0.0
    for nm, o in zip(("xr", "xs", "xd"), outs):
        o = o.float().cpu()
        if ("out/" + nm) in z:
            d = float((o - torch.from_numpy(z["out/" + nm])).abs().max())
        else:
            n = o.shape[-1]
            c0 = n // 2 - 32
            d2 = float((o[:, :, 3::8, 5::8] - torch.from_numpy(z["strided/" + nm])).abs().max())
            d1 = float((o[:, :, c0:c0 + 64, c0:c0 + 64] - torch.from_numpy(z["crop/" + nm])).abs().max()) if ("crop/" + nm) in z else d2
            d = max(d1, d2)
        worst = max(worst, d)
        assert d <= tol, "%s: max-abs %.3e > %.1e" % (nm, d, tol)
    return worst
