#!/usr/bin/env python3
"""What the launch plan of the library named by CFEN_HIP_LIB (default: the built one) does, as JSON: for an A/B of two builds of the same ABI whose host plan
(csrc/cfen_net.cpp) differs and whose device code does not.  Two runs, one per library, must write identical files.
Usage: plan_digest.py OUT.json               on the GPU: per case the (label, class, flops, bytes, kernel) of every launch (net.profile) and the SHA-256 of the
                                             three outputs of an eager forward and of a graph replay
       plan_digest.py --create OUT.json      no GPU: per configuration what a fresh cfen_net_create asks for (workspace bytes, flops per image, parameter names)
       plan_digest.py --compare A.json B.json
       plan_digest.py --enqueue N            on the GPU: host wall time of N eager forwards of the fp16 `tiny` net, where host-side work of the plan would show
Cases (fixtures, kinds and settings of tests/test_hip_variants.py): five fixtures x fp32 / fp16 / chain; every launch-plan setting of NET_CASES and NET_DEAD on
`tiny` and `w32`; the serial plan on `tiny`; uint8 input, uint8 output, fp16 output on `full512`; four probe settings on `tiny` (outputs invalid: labels only)."""
import ctypes, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def compare(a, b):
    A, B = (json.load(open(f))["cases"] for f in (a, b))
    bad = [k for k in sorted(set(A) | set(B)) if A.get(k) != B.get(k)]
    for k in bad:
        print("DIFFERS: %s" % k)
    print("%d cases, %s" % (len(A), "identical" if not bad and open(a).read() == open(b).read() else "%d differ" % len(bad)))
    return 1 if bad else 0


def create_cases():
    """the configurations of tests/test_cabi.py's packed-parameter tests (+ the fragment-stream GViT weights, reserved bit 2, for fp16 v3)"""
    from cfen_vit_dehazing_amd import _lib
    from cfen_vit_dehazing_amd.hipnet import _VARIANT_CODE
    lib = _lib.load()
    shapes = [(24, 4, 8, v, w) for v, w in (("v3", False), ("v3", True), ("cfs", False), ("crs", False), ("v5", False), ("v5", True))]
    shapes += [(nf, hdr, patch, "v3", True) for nf, hdr, patch in ((24, 3, 32), (24, 1, 32), (8, 4, 8), (16, 3, 8), (32, 2, 8))]
    cases = {}
    for nf, hdr, patch, variant, wtile in shapes:
        for dtype in (1, 0):
            for stream in ((0, 4) if dtype == 1 and variant == "v3" else (0,)):
                cc = _lib.NetConfigC(batch=2, n_feats=nf, hidden_dim_ratio=hdr, patch_size=patch, load_size=8 * patch, num_heads=4, dtype=dtype,
                                     reserved=(_VARIANT_CODE[variant] << 8) | (2 if wtile else 0) | stream)
                name = "nf%d hdr%d patch%d %s dtype%d reserved%#x" % (nf, hdr, patch, variant, dtype, cc.reserved)
                h = ctypes.c_void_p()
                if lib.cfen_net_create(ctypes.byref(h), ctypes.byref(cc)) != 0:          # a refused configuration: both builds must refuse it in the same words
                    cases[name] = {"refused": lib.cfen_last_error().decode()}
                    continue
                buf = ctypes.create_string_buffer(1 << 20)
                n = lib.cfen_net_missing_params(h, buf, 1 << 20)
                cases[name] = {"workspace_bytes": lib.cfen_net_workspace_bytes(h), "flops_per_image": lib.cfen_net_flops_per_image(h), "missing": n,
                               "missing_params": buf.value.decode()}
                lib.cfen_net_destroy(h)
    return cases


def build(fixture, kind):
    """the net of a fixture (tests/golden/net_<fixture>.npz) and its input; kind: fp32 / fp16 / chain = fp16 with the GViT weights also packed as fragment streams"""
    from cfen_vit_dehazing_amd.manifest import synthetic_input
    from helpers import load_net_fixture
    from test_hip_net import make_net
    cfg, batch, _ = load_net_fixture(fixture)
    if kind == "chain":
        os.environ["CFEN_GVIT_CHAIN"] = "1"          # read when the net is built
    try:
        net = make_net(cfg, "fp32" if kind == "fp32" else "fp16")
    finally:
        os.environ.pop("CFEN_GVIT_CHAIN", None)
    return net, synthetic_input(batch, cfg).to("cuda:0")


def enqueue_ms(n):
    """host wall time of n eager forwards of the fp16 `tiny` net, synchronised once at the end: the forward is enqueue-bound there, so this is the host plan's own cost"""
    import time
    import torch
    net, x = build("tiny_nf24_hdr4", "fp16")
    for _ in range(20):
        net(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        net(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def gpu_cases():
    import torch
    from cfen_vit_dehazing_amd import ops
    from test_hip_variants import FIXTURES, NET_CASES, NET_DEAD, PLAN_FIXTURES as PLAN_NAMES
    PLAN_FIXTURES = {short: FIXTURES[short] for short in PLAN_NAMES}          # "tiny", and "w32": the 32-pixel windows the window and D = 384 stream kernels need

    def sha(outs):
        torch.cuda.synchronize()
        return [hashlib.sha256(o.contiguous().cpu().numpy().tobytes()).hexdigest() for o in outs]

    def launches(net, x):
        return [[l[0], l[1], l[2], l[5], l[4]] for l in net.profile(x)["launches"]]

    def digest(net, x):
        d = {"launches": launches(net, x), "eager": sha(net(x))}
        gid, outs = net.capture(x)
        net.replay(gid)
        d["graph"] = sha(outs)
        return d

    cases, kept = {}, {}
    for fixture in ("tiny_nf24_hdr4", "cfs_full256_nf24_hdr4", "full512_nf24_hdr4", "v5_tiny_nf24_hdr4", "crs_tiny_nf24_hdr4"):
        for kind in ("fp32", "fp16", "chain"):
            net, x = build(fixture, kind)
            cases["%s %s" % (fixture, kind)] = digest(net, x)
            print("%s %s: %d launches" % (fixture, kind, len(cases["%s %s" % (fixture, kind)]["launches"])), flush=True)
            if fixture in PLAN_FIXTURES.values():
                kept[fixture, kind] = (net, x)
            elif fixture.startswith("full512") and kind == "fp16":
                x8 = ((x.clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
                cases["full512 fp16 uint8 input"] = digest(net, x8)
                for attr in ("output_u8", "output_f16"):
                    setattr(net, attr, True)
                    cases["full512 fp16 %s" % attr] = digest(net, x)
                    setattr(net, attr, False)
            del net
            torch.cuda.empty_cache()
    for key, value, kind in list(dict.fromkeys(list(NET_CASES) + list(NET_DEAD))):
        for short, fixture in PLAN_FIXTURES.items():
            with ops.tuning({key: value}):
                cases["%s %s %s=%d" % (short, kind, key, value)] = digest(*kept[fixture, kind])
    net, x = kept[PLAN_FIXTURES["tiny"], "fp16"]
    for probe in ({"net.skip_from": 10, "net.skip_to": 20}, {"net.skip_classes": 8}, {"net.extra_launches": 2}, {"net.gvit_dummy_wgs": 8}):
        with ops.tuning(probe):
            cases["tiny fp16 probe %s" % ",".join("%s=%d" % kv for kv in probe.items())] = {"labels": [l[0] for l in launches(net, x)]}
        torch.cuda.synchronize()
    net.serial_plan = True
    cases["tiny fp16 serial_plan"] = digest(net, x)
    return cases


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1] == "--enqueue":
        print("%d eager forwards: %.2f ms" % (int(sys.argv[2]), enqueue_ms(int(sys.argv[2]))))
        sys.exit(0)
    cases = create_cases() if sys.argv[1] == "--create" else gpu_cases()
    with open(sys.argv[-1], "w") as f:
        json.dump({"cases": cases}, f, indent=1, sort_keys=True)
    from cfen_vit_dehazing_amd import _lib
    print("%d cases of %s -> %s" % (len(cases), _lib.LIB_PATH, sys.argv[-1]))
