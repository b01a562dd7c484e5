#!/usr/bin/env python3
"""Cost of the per-plane scores against a ground-truth stream (cfen_plane_metrics, csrc/k_planes.hip) beside ops.image_metrics on the same
number of samples and beside a plain copy of the bytes it reads.

    python tools/bench_plane_metrics.py [--out profiles/plane_metrics_bench.json] [--iters 100 --reps 7]

Shapes: eight 512 x 512 C420jpeg frames (8 bits) and one 2160 x 3840 C420p10 frame (4:2:0 co-sited, 10 bits).  One child process under its own
time limit measures, per shape and in the same run:
  plane_metrics   ops.plane_metrics with a previous frame pair (so the temporal term reads its two extra frames for frame 0), us per call
  image_metrics   ops.image_metrics on (B, Hs, W, 3) uint8 images holding as many samples as the frames: Hs = samples per frame / (3 W).  The
                  same tile and the same passes on as many values, from bytes in one interleaved plane
  copy            a device-to-device copy of the bytes plane_metrics reads: both streams and, through the temporal term, each frame's predecessor
                  pair, i.e. 4 B frame_bytes
  call_floor      ops.plane_metrics on one 11 x 11 mono frame: what a call costs when the kernels have one tile (the wrapper and two launches)
Timing: device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"512x512_batch8_420jpeg": (8, 512, 512, "420jpeg", 8), "2160x3840_420p10": (1, 2160, 3840, "420mpeg2", 10)}
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
    from cfen_vit_dehazing_amd import ops, yuv
    res = {}
    for name, (B, H, W, chroma, depth) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        nb = yuv.frame_bytes(H, W, chroma, depth)

        def stream(n):
            if depth == 8:
                return torch.randint(0, 256, (n, nb), generator=g, dtype=torch.uint8).cuda()
            return torch.randint(0, 1 << depth, (n, nb // 2), generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint8).reshape(n, nb).cuda()
        a, b = stream(B + 1), stream(B + 1)
        samples = nb // (2 if depth > 8 else 1)
        Hs = samples // (3 * W)
        ia = torch.randint(0, 256, (B, Hs, W, 3), generator=g, dtype=torch.uint8).cuda()
        ib = torch.randint(0, 256, (B, Hs, W, 3), generator=g, dtype=torch.uint8).cuda()
        total = 4 * B * nb
        src, dst = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
        r = {"plane_metrics": _timed(lambda: ops.plane_metrics(a[1:], b[1:], H, W, chroma, depth, prev=(a[0], b[0])), args.iters, args.reps),
             "image_metrics": _timed(lambda: ops.image_metrics(ia, ib), args.iters, args.reps),
             "copy": _timed(lambda: dst.copy_(src), args.iters, args.reps)}
        r["bytes_read"] = total
        r["samples_per_frame"], r["image_metrics_shape"] = samples, [B, Hs, W, 3]
        r["plane_metrics_over_image_metrics"] = round(r["plane_metrics"]["us_median"] / r["image_metrics"]["us_median"], 2)
        r["plane_metrics_over_copy"] = round(r["plane_metrics"]["us_median"] / r["copy"]["us_median"], 2)
        r["plane_metrics_gsamples_per_s"] = round(B * samples / r["plane_metrics"]["us_median"] / 1e3, 2)
        r["image_metrics_gsamples_per_s"] = round(B * Hs * W * 3 / r["image_metrics"]["us_median"] / 1e3, 2)
        res[name] = r
    tiny = torch.zeros(1, 121, dtype=torch.uint8, device="cuda")
    res["call_floor"] = _timed(lambda: ops.plane_metrics(tiny, tiny, 11, 11, "mono", 8), args.iters, args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_metrics_bench.json"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_plane_metrics.py needs a GPU")
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
