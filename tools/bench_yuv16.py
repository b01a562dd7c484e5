#!/usr/bin/env python3
"""Cost of the deep YCbCr <-> float RGB conversions (cfen_yuv16_to_rgb_f32 / cfen_rgb_f32_to_yuv16, csrc/k_yuv16.hip) beside a plain copy of the
same number of bytes.

    python tools/bench_yuv16.py [--out profiles/yuv16_bench.json] [--iters 100 --reps 7]

Shapes: eight 512 x 512 frames -- the benchmark batch -- and one 2160 x 3840 frame, C420p10 (4:2:0 co-sited, 10 bits), bt709 limited.  One child
process under its own time limit measures, per shape and in the same run:
  yuv16_to_rgb   ops.yuv16_to_rgb_f32 into a preallocated output, us per call
  rgb_to_yuv16   ops.rgb_f32_to_yuv16 into a preallocated output
  copy           a device-to-device copy of frame_bytes + 12 H W bytes per frame: the bytes either direction reads and writes
  call_floor     ops.yuv16_to_rgb_f32 on one 2 x 2 frame: what a call costs when the kernel has nothing to do (the Python wrapper and the launch)
Timing: device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups.  One batch per shape: the 512 x 512
batch (28 MB both ways) stays in the caches, the 2160 x 3840 frame (112 MB) partly; the copy of the same bytes in the same run is the yardstick."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"512x512_batch8": (8, 512, 512), "2160x3840": (1, 2160, 3840)}
CHROMA, DEPTH, MATRIX, FULL = "420mpeg2", 10, "bt709", False
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
    for name, (B, H, W) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        nb = yuv.frame_bytes(H, W, CHROMA, DEPTH)
        samples = torch.randint(0, 1 << DEPTH, (B, nb // 2), generator=g, dtype=torch.int32).to(torch.int16)
        frames = samples.view(torch.uint8).reshape(B, nb).cuda()
        rgb = (torch.rand((B, 3, H, W), generator=g, dtype=torch.float32) * 2 - 1).cuda()
        out_rgb, out_frames = torch.empty_like(rgb), torch.empty_like(frames)
        total = B * (nb + 12 * H * W)
        src, dst = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
        r = {"yuv16_to_rgb": _timed(lambda: ops.yuv16_to_rgb_f32(frames, H, W, CHROMA, DEPTH, MATRIX, FULL, out=out_rgb), args.iters, args.reps),
             "rgb_to_yuv16": _timed(lambda: ops.rgb_f32_to_yuv16(rgb, CHROMA, DEPTH, MATRIX, FULL, out=out_frames), args.iters, args.reps),
             "copy": _timed(lambda: dst.copy_(src), args.iters, args.reps)}
        r["bytes_read_and_written"] = total
        for k in ("yuv16_to_rgb", "rgb_to_yuv16"):
            r[k + "_over_copy"] = round(r[k]["us_median"] / r["copy"]["us_median"], 2)
            r[k + "_gbytes_per_s"] = round(total / r[k]["us_median"] / 1e3, 1)
        r["copy_gbytes_per_s"] = round(total / r["copy"]["us_median"] / 1e3, 1)
        res["%s_420p%d" % (name, DEPTH)] = r
    tiny, tiny_out = torch.zeros(1, yuv.frame_bytes(2, 2, CHROMA, DEPTH), dtype=torch.uint8, device="cuda"), torch.empty(1, 3, 2, 2, dtype=torch.float32, device="cuda")
    res["call_floor"] = _timed(lambda: ops.yuv16_to_rgb_f32(tiny, 2, 2, CHROMA, DEPTH, MATRIX, FULL, out=tiny_out), args.iters, args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv16_bench.json"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_yuv16.py needs a GPU")
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
