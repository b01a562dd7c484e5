#!/usr/bin/env python3
"""Cost of scoring (cfen_image_metrics, csrc/k_metrics.hip) beside a torch restatement of the same definition and beside the forward it scores.

    python tools/bench_metrics.py [--out profiles/metrics_bench.json] [--iters 200 --reps 7]

Shapes: uint8 (8,512,512,3) -- the benchmark batch -- and one 2160 x 3840 pair.  Three steps, each a child process of its own under its own time
limit (a step that fails or runs over ends the tool; nothing else is started on the device after it):
  kernel   ops.image_metrics (both launches of the call), us per call
  torch    the definition restated with torch on the same device: v / 255, five grouped F.conv2d with the 11 x 11 window, the SSIM map, two means
  forward  the fp16 generator forward of the same (8,512,512,3) uint8 batch with uint8 outputs, ms -- what one scored batch costs to produce
Timing: device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups.  Each is measured twice: on ONE input
pair (it stays in the caches) and rotating over pairs that together exceed the 256 MB last-level cache (every call reads its images from HBM)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"512x512_batch8": (8, 512, 512), "2160x3840": (1, 2160, 3840)}
STEP_TIMEOUT_S = {"kernel": 240, "torch": 240, "forward": 300}


def _timed(fn, n_inputs, iters, reps):
    import torch
    for i in range(max(10, n_inputs)):
        fn(i % n_inputs)
    torch.cuda.synchronize()
    groups = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(i % n_inputs)
        e1.record()
        e1.synchronize()
        groups.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"us_median": round(statistics.median(groups), 2), "us_min": round(min(groups), 2), "us_max": round(max(groups), 2)}


def _pairs(shape, n):
    import torch
    B, H, W = shape
    g = torch.Generator().manual_seed(0)
    return [(torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda(), torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda())
            for _ in range(n)]


def _rotation(shape):
    B, H, W = shape
    return -(-(320 << 20) // (2 * B * H * W * 3))          # pairs whose bytes pass 320 MB


def step_kernel(args):
    import torch
    from cfen_vit_dehazing_amd import ops
    res = {}
    for name, shape in SHAPES.items():
        pairs = _pairs(shape, _rotation(shape))
        out = torch.empty(shape[0], 2, dtype=torch.float64, device="cuda")
        fn = lambda i: ops.image_metrics(pairs[i][0], pairs[i][1], out=out)      # noqa: E731
        res[name] = {"one_pair": _timed(fn, 1, args.iters, args.reps), "rotating": dict(_timed(fn, len(pairs), args.iters, args.reps), pairs=len(pairs))}
    return res


def _torch_ssim_psnr(a, b, window):
    import torch.nn.functional as F
    x, y = a.permute(0, 3, 1, 2).float() / 255.0, b.permute(0, 3, 1, 2).float() / 255.0
    mu1, mu2 = F.conv2d(x, window, groups=3), F.conv2d(y, window, groups=3)
    s11 = F.conv2d(x * x, window, groups=3) - mu1 * mu1
    s22 = F.conv2d(y * y, window, groups=3) - mu2 * mu2
    s12 = F.conv2d(x * y, window, groups=3) - mu1 * mu2
    m = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    return ((x - y) ** 2).mean(dim=(1, 2, 3)), m.mean(dim=(1, 2, 3))


def step_torch(args):
    import math
    import torch
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float64)
    g = g / g.sum()
    window = (g[:, None] * g[None, :]).float().expand(3, 1, 11, 11).contiguous().cuda()
    res = {}
    for name, shape in SHAPES.items():
        pairs = _pairs(shape, _rotation(shape))
        fn = lambda i: _torch_ssim_psnr(pairs[i][0], pairs[i][1], window)       # noqa: E731
        iters = max(10, args.iters // 10)
        res[name] = {"one_pair": _timed(fn, 1, iters, args.reps), "rotating": dict(_timed(fn, len(pairs), iters, args.reps), pairs=len(pairs))}
    return res


def step_forward(args):
    import torch
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    from cfen_vit_dehazing_amd.manifest import generate_state_dict
    cfg = NetConfig(24, 4, patch_size=32, load_size=256)
    net = dec_ipt(cfg, compute_dtype="fp16")
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to("cuda:0")
    net.output_u8 = True
    x = _pairs(SHAPES["512x512_batch8"], 1)[0][0]
    with torch.no_grad():
        t = _timed(lambda i: net(x), 1, max(10, args.iters // 10), args.reps)
    return {"512x512_batch8": {"ms_median": round(t["us_median"] / 1e3, 3), "ms_min": round(t["us_min"] / 1e3, 3), "ms_max": round(t["us_max"] / 1e3, 3),
                               "what": "fp16 forward, uint8 in, uint8 out, eager launches"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT_S), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_metrics.py needs a GPU")
        print("RESULT " + json.dumps({"kernel": step_kernel, "torch": step_torch, "forward": step_forward}[args.step](args)))
        return
    record = {"iters": args.iters, "reps": args.reps}
    for step in ("kernel", "torch", "forward"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--iters", str(args.iters), "--reps", str(args.reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_TIMEOUT_S[step])
        except subprocess.TimeoutExpired:
            raise SystemExit("step %s ran over its %d s limit: stopping" % (step, STEP_TIMEOUT_S[step]))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            raise SystemExit("step %s failed (exit %d): stopping\n%s" % (step, r.returncode, r.stdout[-2000:]))
        record[step] = json.loads(lines[-1][7:])
        print(step, json.dumps(record[step]), flush=True)
    try:
        import torch
        record["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else None
    except Exception:
        record["device"] = None
    k, t = record["kernel"]["512x512_batch8"]["rotating"]["us_median"], record["torch"]["512x512_batch8"]["rotating"]["us_median"]
    record["summary_512x512_batch8"] = {"kernel_us": k, "torch_restatement_us": t, "forward_ms": record["forward"]["512x512_batch8"]["ms_median"],
                                        "kernel_share_of_forward_pct": round(100 * k / 1e3 / record["forward"]["512x512_batch8"]["ms_median"], 2)}
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record["summary_512x512_batch8"]))


if __name__ == "__main__":
    main()
