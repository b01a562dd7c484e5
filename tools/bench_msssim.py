#!/usr/bin/env python3
"""Cost of MS-SSIM scoring (cfen_image_msssim, csrc/k_metrics.hip) beside cfen_image_metrics on the same inputs, beside a torch restatement of the
same definition, and beside the forward it scores.

    python tools/bench_msssim.py [--out profiles/msssim_bench.json] [--iters 200 --reps 7]

Shapes, timing and the one-pair / rotating inputs are those of tools/bench_metrics.py (its helpers are imported): uint8 (8,512,512,3) and one
2160 x 3840 pair; device events around `iters` back-to-back calls, after a warm-up; the median of `reps` such groups.  Steps, each a child process
of its own under its own time limit (a step that fails or runs over ends the tool; nothing else is started on the device after it):
  kernel   ops.image_msssim (five level launches and the finish) and, in the same process on the same inputs, ops.image_metrics
  torch    the definition restated with torch: per level five grouped F.conv2d with the 11 x 11 window, the SSIM and cs maps, their means, and
           F.avg_pool2d of both images between levels
  forward  the fp16 generator forward of the same (8,512,512,3) uint8 batch with uint8 outputs (bench_metrics.step_forward)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_metrics as bm  # noqa: E402

STEP_TIMEOUT_S = {"kernel": 300, "torch": 300, "forward": 300}


def step_kernel(args):
    import torch
    from cfen_vit_dehazing_amd import ops
    res = {}
    for name, shape in bm.SHAPES.items():
        pairs = bm._pairs(shape, bm._rotation(shape))
        out = torch.empty(shape[0], 11, dtype=torch.float64, device="cuda")
        out2 = torch.empty(shape[0], 2, dtype=torch.float64, device="cuda")
        ms = lambda i: ops.image_msssim(pairs[i][0], pairs[i][1], out=out)      # noqa: E731
        one = lambda i: ops.image_metrics(pairs[i][0], pairs[i][1], out=out2)    # noqa: E731
        res[name] = {"msssim": {"one_pair": bm._timed(ms, 1, args.iters, args.reps),
                                "rotating": dict(bm._timed(ms, len(pairs), args.iters, args.reps), pairs=len(pairs))},
                     "image_metrics": {"one_pair": bm._timed(one, 1, args.iters, args.reps),
                                       "rotating": dict(bm._timed(one, len(pairs), args.iters, args.reps), pairs=len(pairs))}}
    return res


def _torch_msssim(a, b, window):
    import torch
    import torch.nn.functional as F
    x, y = a.permute(0, 3, 1, 2).float() / 255.0, b.permute(0, 3, 1, 2).float() / 255.0
    sse = ((x - y) ** 2).sum(dim=(1, 2, 3))
    levels = []
    for l in range(5):
        mu1, mu2 = F.conv2d(x, window, groups=3), F.conv2d(y, window, groups=3)
        s11 = F.conv2d(x * x, window, groups=3) - mu1 * mu1
        s22 = F.conv2d(y * y, window, groups=3) - mu2 * mu2
        s12 = F.conv2d(x * y, window, groups=3) - mu1 * mu2
        v1, v2 = 2 * s12 + 9e-4, s11 + s22 + 9e-4
        m = ((2 * mu1 * mu2 + 1e-4) * v1) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * v2)
        levels.append(torch.stack([m.mean(dim=(1, 2, 3)), (v1 / v2).mean(dim=(1, 2, 3))], dim=1))
        if l < 4:
            x, y = F.avg_pool2d(x, (2, 2)), F.avg_pool2d(y, (2, 2))
    return sse, torch.stack(levels, dim=1)


def step_torch(args):
    import math
    import torch
    g = torch.tensor([math.exp(-(i - 5) ** 2 / 4.5) for i in range(11)], dtype=torch.float64)
    g = g / g.sum()
    window = (g[:, None] * g[None, :]).float().expand(3, 1, 11, 11).contiguous().cuda()
    res = {}
    for name, shape in bm.SHAPES.items():
        pairs = bm._pairs(shape, bm._rotation(shape))
        fn = lambda i: _torch_msssim(pairs[i][0], pairs[i][1], window)       # noqa: E731
        iters = max(10, args.iters // 10)
        res[name] = {"one_pair": bm._timed(fn, 1, iters, args.reps), "rotating": dict(bm._timed(fn, len(pairs), iters, args.reps), pairs=len(pairs))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msssim_bench.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT_S), help="(internal) run one step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bench_msssim.py needs a GPU")
        print("RESULT " + json.dumps({"kernel": step_kernel, "torch": step_torch, "forward": bm.step_forward}[args.step](args)))
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
    for name in bm.SHAPES:
        k = record["kernel"][name]["msssim"]["rotating"]["us_median"]
        one = record["kernel"][name]["image_metrics"]["rotating"]["us_median"]
        t = record["torch"][name]["rotating"]["us_median"]
        record["summary_" + name] = {"msssim_us": k, "image_metrics_us": one, "ratio_to_image_metrics": round(k / one, 2), "torch_restatement_us": t,
                                     "torch_over_kernel": round(t / k, 1)}
    fwd = record["forward"]["512x512_batch8"]["ms_median"]
    record["summary_512x512_batch8"].update(forward_ms=fwd, msssim_share_of_forward_pct=round(100 * record["summary_512x512_batch8"]["msssim_us"] / 1e3 / fwd, 2))
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: v for k, v in record.items() if k.startswith("summary_")}))


if __name__ == "__main__":
    main()
