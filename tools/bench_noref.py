#!/usr/bin/env python3
"""Cost of the no-reference statistics (cfen_noref_u8, csrc/k_noref.hip) beside the PSNR / SSIM pass and a plain copy of the same bytes.

    python tools/bench_noref.py [--out profiles/noref_bench.json] [--iters 100 --reps 7]

Shapes: uint8 (8,512,512,3) -- the benchmark batch -- and one 2160 x 3840 pair, radius 7.  One child process under its own time limit measures, per
shape and in the same run:
  noref          ops.image_noref without the maps (both launches of the call), us per call
  noref_maps     the same with the two (B,H,W) uint8 dark-channel maps written
  noref_r16      without the maps at radius 16, the largest window
  image_metrics  ops.image_metrics on the same inputs (both launches): the yardstick the scores sit beside
  copy           a device-to-device copy of both images' bytes: what touching the inputs once costs
Timing: device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups.  The inputs stay in the caches (one
pair per shape), so the copy is the generous yardstick."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"512x512_batch8": (8, 512, 512), "2160x3840": (1, 2160, 3840)}
RADIUS = 7
STEP_TIMEOUT_S = 240


def _timed(fn, iters, reps):
    import torch
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    groups = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        groups.append(e0.elapsed_time(e1) * 1e3 / iters)
    return {"us_median": round(statistics.median(groups), 2), "us_min": round(min(groups), 2), "us_max": round(max(groups), 2)}


def step_measure(args):
    import torch
    from cfen_vit_dehazing_amd import ops
    res = {}
    for name, (B, H, W) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        a = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        b = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        out2 = torch.empty(B, 2, dtype=torch.float64, device="cuda")
        both, dst = torch.stack([a, b]), torch.empty(2, B, H, W, 3, dtype=torch.uint8, device="cuda")
        r = {"noref": _timed(lambda: ops.image_noref(a, b, radius=RADIUS), args.iters, args.reps),
             "noref_maps": _timed(lambda: ops.image_noref(a, b, radius=RADIUS, maps=True), args.iters, args.reps),
             "noref_r16": _timed(lambda: ops.image_noref(a, b, radius=16), args.iters, args.reps),
             "image_metrics": _timed(lambda: ops.image_metrics(a, b, out=out2), args.iters, args.reps),
             "copy": _timed(lambda: dst.copy_(both), args.iters, args.reps)}
        px = B * H * W
        r["pixels"] = px
        r["bytes_read"] = 6 * px
        r["noref_ns_per_pixel"] = round(r["noref"]["us_median"] * 1e3 / px, 4)
        r["noref_gpixels_per_s"] = round(px / r["noref"]["us_median"] / 1e3, 2)
        r["noref_over_image_metrics"] = round(r["noref"]["us_median"] / r["image_metrics"]["us_median"], 2)
        r["noref_over_copy"] = round(r["noref"]["us_median"] / r["copy"]["us_median"], 2)
        r["noref_share_of_copy_rate"] = round(r["copy"]["us_median"] / r["noref"]["us_median"], 4)
        res[name] = r
    res["device"] = torch.cuda.get_device_name(0)
    res["radius"] = RADIUS
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noref_bench.json"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_noref.py needs a GPU")
        print("RESULT " + json.dumps(step_measure(args)))
        return
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "measure", "--iters", str(args.iters), "--reps", str(args.reps)]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=STEP_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit("the measurement ran over its %d s limit: stopping" % STEP_TIMEOUT_S)
    lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not lines:
        raise SystemExit("the measurement failed (exit %d): stopping\n%s" % (r.returncode, r.stdout[-2000:]))
    record = dict(json.loads(lines[-1][7:]), iters=args.iters, reps=args.reps)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(record, sort_keys=True))


if __name__ == "__main__":
    main()
