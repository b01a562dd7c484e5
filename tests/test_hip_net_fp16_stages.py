"""Every stage of the fp16 forward against a rounding-model bar.

The fp16 plan is what ships and what the benchmark times, and the only plan that runs the fp16-only kernels (the fused window kernel, the streamed
mlp3 / front3 kernels, head5, the Toeplitz 7x7 and rows-layout convolutions, the fused tail, the few-token GViT GEMMs).  test_hip_net.py holds its three
outputs to FP16_BAR; an output bar cannot see a block that is wrong by a few percent (a softmax scale off by 15 % moves the outputs by 4e-3 .. 7e-3).
Here every stage map is compared with the exact result, and the distance may be FP16_STAGE_MARGIN times what the rounding model of the oracle
(cfen_oracle.forward(quant=...), recorded in golden/fp16_stage_model.json by tools/gen_fp16_stage_model.py) has at that stage -- two figures per
stage: the relative rms error, and the largest error.  tests/test_fp16_stage_model_host.py shows on the CPU that wiring mistakes inside a block land
above this bar.

  small fixtures   whole tensors against the float64 oracle run here (every image of the batch on its own)
  full-size ones   the fixture's 512 samples per stage of the reference's own forward, and its abs-sum checksum
  the shipped plan the same with every knob at its default; the stages that plan does not store must be us_conv_d01* (inside the fused tail) and,
                   with "net.up_fused", the GViT maps left at low resolution -- nothing else
  batch 2          at full size, the two images' samples apart
"""
import pytest
import torch

import cfen_oracle
from cfen_vit_dehazing_amd import ops
from cfen_vit_dehazing_amd._lib import CfenError
from cfen_vit_dehazing_amd.manifest import synthetic_input
from helpers import load_net_fixture, weight_mode, sample_idx, gpu_stages, _cfs_stages, fp16_stage_model, FP16_STAGE_MARGIN as MARGIN
from helpers import knobs_at_shipped_defaults  # noqa: F401  (autouse: every knob is back at its shipped default after each test)
from test_hip_net import cached_state_dict, make_net, OFF_NF24

pytestmark = pytest.mark.gpu

SMALL = ["tiny_nf24_hdr4", "tiny_nf24_hdr2", "small_nf24_hdr4"] + OFF_NF24 + ["cfs_tiny_nf24_hdr4", "crs_tiny_nf24_hdr4", "v5_tiny_nf24_hdr4",
                                                                              "refinit_tiny_nf24_hdr4"]
FULL = ["full512_nf24_hdr4", "full512_nf32_hdr6"]
OUTPUTS = ("tail_R", "tail_S", "tail_D")


@pytest.fixture(scope="module")
def model():
    return fp16_stage_model()


def _state_dict(name, cfg, z):
    """the fixture's weights; refinit_*: with the ActNorm parameters of the reference's first forward, so that the net, the oracle and the model
    normalise with the same tables (as test_reference_init_weights_fp16_psnr_ssim_full512 does)"""
    sd = cached_state_dict(cfg, mode=weight_mode(name))
    if "actnorm_names" in z:
        sd = dict(sd)
        for k in [str(v) for v in z["actnorm_names"]]:
            sd[k + ".weight"], sd[k + ".bias"] = torch.from_numpy(z["actnorm_w/" + k]), torch.from_numpy(z["actnorm_b/" + k])
            sd[k + ".initialized"] = torch.tensor(1)
    return sd


_EXACT = {}


def _exact(name, cfg, batch, sd):
    """float64 oracle stages of a small fixture, computed once and read by every test that needs them"""
    if name not in _EXACT:
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items() if not k.startswith(("sub_mean", "add_mean"))}
        st = {}
        with torch.no_grad():
            cfen_oracle.forward(sd64, synthetic_input(batch, cfg).double(), cfg.num_heads, cfg.patch_size, stages=st, variant=cfg.variant)
        _EXACT[name] = st
    return _EXACT[name]


def _forward(name, knobs):
    """(cfg, batch, z, stages the plan stored incl. the three outputs, names it refused)"""
    cfg, batch, z = load_net_fixture(name)
    sd = _state_dict(name, cfg, z)
    net = make_net(cfg, "fp16", sd=sd)
    assert net.compute_dtype == torch.float16
    names = [str(s) for s in z["stage_names"]]
    st, refused = {}, []
    with ops.tuning(knobs):
        outs = net(synthetic_input(batch, cfg).to("cuda:0"))
        if knobs.get("net.keep_stages"):
            st = {n: t.cpu() for n, t in (gpu_stages if cfg.variant in ("v3", "v5") else _cfs_stages)(net, z).items()}
        else:                                  # the same reading, stage by stage: this plan does not store every map
            xf = net.stage("head" if cfg.full_res else "ds_conv_e01")
            for n in names:
                if n.startswith("tail_"):
                    continue
                try:
                    t = net.stage(n)
                except CfenError as e:
                    assert "net.keep_stages" in str(e), (n, str(e))     # the refusal of a map the plan did not store, not some other failure
                    refused.append(n)
                    continue
                st[n] = (t - xf if n.startswith("lgcat_conv_d01") else t).cpu()     # the plan stores `stage + xf` there (helpers.gpu_stages)
    for nm, o in zip(OUTPUTS, outs):
        st[nm] = o.float().cpu()
    del net
    torch.cuda.empty_cache()
    return cfg, batch, z, sd, st, refused


def _report(tag, rows):
    """rows: (stage, what, measured, model) -> prints every GPU / model ratio, then fails on those above the margin"""
    worst = max(rows, key=lambda r: r[2] / r[3])
    for n, what, got, mod in rows:
        print("%-26s %-22s %-16s gpu %.3e  model %.3e  ratio %5.2f" % (tag, n, what, got, mod, got / mod))
    print("%s: worst GPU / model ratio %.2f (%s, %s) over %d figures; margin %.1f" % (tag, worst[2] / worst[3], worst[0], worst[1], len(rows), MARGIN))
    bad = [(n, what, "%.3e" % got, "%.3e" % mod, "%.2f" % (got / mod)) for n, what, got, mod in rows if not got <= MARGIN * mod]
    assert not bad, "%s: stages outside %.1f x the rounding model (stage, figure, gpu, model, ratio): %r" % (tag, MARGIN, bad)


def _whole_tensor_rows(st, exact, table, batch):
    rows = []
    for n, t in st.items():
        ex = exact[n]
        assert tuple(t.shape) == tuple(ex.shape), n
        rms = float(ex.pow(2).mean().sqrt())
        assert abs(rms - table[n]["rms"]) <= 1e-6 * rms, n                     # the table was made for this fixture's weights and input
        for b in range(batch):
            d = t[b].double() - ex[b]
            tag = "" if batch == 1 else " img%d" % b
            rows.append((n, "rel rms" + tag, float(d.pow(2).mean().sqrt()) / rms, table[n]["rel_rms"]))
            rows.append((n, "max abs" + tag, float(d.abs().max()), table[n]["max_abs"]))
    return rows


def _sample_rows(st, z, table, batch, per_image=False):
    rows = []
    for n, t in st.items():
        assert tuple(t.shape) == tuple(int(v) for v in z["stage_shape/" + n]), n
        idx = sample_idx(n, t.numel())
        ref = torch.from_numpy(z["stage_smp/" + n]).double()
        d = t.flatten()[idx].double() - ref
        rms = float(ref.pow(2).mean().sqrt())
        groups = [("", torch.ones_like(idx, dtype=torch.bool))]
        if per_image:
            img = idx // (t.numel() // batch)
            groups = [(" img%d" % b, img == b) for b in range(batch)]
        for tag, m in groups:
            assert int(m.sum()) >= 128, (n, tag)
            rows.append((n, "rel rms smp" + tag, float(d[m].pow(2).mean().sqrt()) / rms, table[n]["rel_rms_smp"]))
            rows.append((n, "max abs smp" + tag, float(d[m].abs().max()), table[n]["max_abs_smp"]))
        ref_abs = float(z["stage_abs/" + n])
        rows.append((n, "abs-sum", abs(float(t.double().abs().sum()) - ref_abs) / ref_abs, table[n]["rel_rms"]))
    return rows


@pytest.mark.parametrize("name", SMALL)
def test_fp16_every_stage_of_the_small_fixtures_whole_tensors(model, name):
    cfg, batch, z, sd, st, refused = _forward(name, {"net.keep_stages": 1})
    assert not refused and len(st) == len(z["stage_names"])
    _report(name, _whole_tensor_rows(st, _exact(name, cfg, batch, sd), model[name], batch))


@pytest.mark.parametrize("name", FULL)
def test_fp16_every_stage_of_the_full_size_fixtures_at_the_reference_samples(model, name):
    cfg, batch, z, sd, st, refused = _forward(name, {"net.keep_stages": 1})
    assert not refused and len(st) == len(z["stage_names"])
    _report(name, _sample_rows(st, z, model[name], batch))


UP = {"net.up_fused": 1}


@pytest.mark.parametrize("name,knobs", [("full512_nf24_hdr4", {}), ("full512_nf32_hdr6", {}), ("tiny_nf24_hdr4", {}), ("small_nf24_hdr4", {}),
                                        ("full512_nf24_hdr4", UP), ("tiny_nf24_hdr4", UP)], ids=lambda v: v if isinstance(v, str) else "+".join(v) or "shipped")
def test_fp16_every_stage_the_shipped_plan_stores(model, name, knobs):
    """every knob at its default: the fused window / stream / tail launches, which the "net.keep_stages" plan of the tests above replaces in part.  That plan
    does not store every map, and cfen_net_stage refuses the ones it did not store.  With the shipped knobs those must be exactly us_conv_d01* (inside the fused
    tail).  With "net.up_fused" (x4 bilinear of the GViT result inside the level's fuse conv; off as shipped, csrc/cfen_tune_knobs.hpp) the GViT maps stay at
    low resolution too: refusals may then only be globalvit_* and us_conv_d01*, and at the benchmarked configuration they are all of those, 12 + 3.
    Every other stage is read and held to the same bar."""
    cfg, batch, z, sd, st, refused = _forward(name, knobs)
    print("%s, knobs %r: not stored: %s" % (name, knobs, ", ".join(refused) or "nothing"))
    names = [str(s) for s in z["stage_names"]]
    tail_maps = sorted(n for n in names if n.startswith("us_conv_d01"))
    gvit_maps = sorted(n for n in names if n.startswith("globalvit_"))
    assert len(tail_maps) == 3 and len(gvit_maps) == 12
    if not knobs:
        assert sorted(refused) == tail_maps
    else:
        assert set(tail_maps) <= set(refused) <= set(tail_maps + gvit_maps), "the plan refuses stages it should store: %r" % sorted(set(refused) - set(tail_maps + gvit_maps))
        if name == "full512_nf24_hdr4":
            assert sorted(refused) == sorted(tail_maps + gvit_maps)
    assert len(st) + len(refused) == len(names)
    tag = "%s (%s)" % (name, "+".join(knobs) or "shipped")
    if name.startswith("full512"):
        _report(tag, _sample_rows(st, z, model[name], batch))
    else:
        _report(tag, _whole_tensor_rows(st, _exact(name, cfg, batch, sd), model[name], batch))


def test_fp16_every_stage_of_both_images_at_batch_2(model):
    """512 x 512, two images (seeds 0 and 1), against the reference's own batch-2 forward: the samples of each image are held to the bar on their own, so a
    stage indexed with the wrong image stride shows up in the second image"""
    name = "full512b2_nf24_hdr4"
    cfg, batch, z, sd, st, refused = _forward(name, {"net.keep_stages": 1})
    assert batch == 2 and not refused and len(st) == len(z["stage_names"])
    _report(name, _sample_rows(st, z, model[name], batch, per_image=True))
