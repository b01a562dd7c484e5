#!/usr/bin/env python3
"""Cost of the YCbCr <-> RGB conversions (cfen_yuv_to_rgb_u8 / cfen_rgb_to_yuv_u8, csrc/k_yuv.hip) beside a plain copy of the same bytes.

    python tools/bench_yuv.py [--out profiles/yuv_bench.json] [--iters 100 --reps 7]

Shapes: eight 512 x 512 frames -- the benchmark batch -- and one 2160 x 3840 frame, 4:2:0 (420jpeg, and 420mpeg2 for the co-sited filters), bt709
limited.  One child process under its own time limit measures, per shape and in the same run:
  yuv_to_rgb   ops.yuv_to_rgb_u8 into a preallocated output, us per call
  rgb_to_yuv   ops.rgb_to_yuv_u8 into a preallocated output
  copy         a device-to-device copy of frame_bytes + 3 H W bytes per frame: the bytes either direction reads and writes
  call_floor   ops.yuv_to_rgb_u8 on one 2 x 2 frame: what a call costs when the kernel has nothing to do (the Python wrapper and the launch);
               a shape whose time is near this floor is bound by the host issuing the calls, not by the kernel
Timing: device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups.  The buffers stay in the caches (one
batch per shape), so the copy is the generous yardstick."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"512x512_batch8": (8, 512, 512), "2160x3840": (1, 2160, 3840)}
CHROMAS = ("420jpeg", "420mpeg2")
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
        for chroma in CHROMAS:
            g = torch.Generator().manual_seed(0)
            nb = yuv.frame_bytes(H, W, chroma)
            frames = torch.randint(0, 256, (B, nb), generator=g, dtype=torch.uint8).cuda()
            rgb = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
            out_rgb, out_frames = torch.empty_like(rgb), torch.empty_like(frames)
            total = B * (nb + 3 * H * W)
            src, dst = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
            r = {"yuv_to_rgb": _timed(lambda: ops.yuv_to_rgb_u8(frames, H, W, chroma, "bt709", False, out=out_rgb), args.iters, args.reps),
                 "rgb_to_yuv": _timed(lambda: ops.rgb_to_yuv_u8(rgb, chroma, "bt709", False, out=out_frames), args.iters, args.reps),
                 "copy": _timed(lambda: dst.copy_(src), args.iters, args.reps)}
            r["bytes_read_and_written"] = total
            for k in ("yuv_to_rgb", "rgb_to_yuv"):
                r[k + "_over_copy"] = round(r[k]["us_median"] / r["copy"]["us_median"], 2)
                r[k + "_gbytes_per_s"] = round(total / r[k]["us_median"] / 1e3, 1)
            r["copy_gbytes_per_s"] = round(total / r["copy"]["us_median"] / 1e3, 1)
            res["%s_%s" % (name, chroma)] = r
    tiny, tiny_out = torch.zeros(1, yuv.frame_bytes(2, 2, "420jpeg"), dtype=torch.uint8, device="cuda"), torch.empty(1, 2, 2, 3, dtype=torch.uint8, device="cuda")
    res["call_floor"] = _timed(lambda: ops.yuv_to_rgb_u8(tiny, 2, 2, "420jpeg", "bt709", False, out=tiny_out), args.iters, args.reps)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.json"))
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=["measure"], help="(internal) run the measurement in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_yuv.py needs a GPU")
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
