#!/usr/bin/env python3
"""Cost of the geometric self-ensemble (ensemble.py): ms per image of forward_x8 next to the plain batch-8 forward of the same process, the
expand + merge kernel pair alone (microseconds, and effective GB/s against the 6.29 TB/s measured copy rate of MI355X HBM), and the same glue
written with torch ops (8 flips / transposes and a stack in front; 21 inverse transforms, the ordered sums and the scaling behind).

    python tools/bench_ensemble.py [--dtype fp16 --load-size 256 --u8 --out profiles/ensemble_bench.json]

Device events around each phase, every phase warmed up first, the median of 7.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from cfen_vit_dehazing_amd import ops
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict

COPY_TBPS = 6.29          # MI355X_MICROARCH.md: measured device-to-device copy rate
REPS = 7


def timed(fn, inner=1):
    """median over REPS of the device time of `inner` back-to-back calls of fn, per call, in ms"""
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return sorted(ms)[len(ms) // 2]


def torch_expand(img, u8):
    H, W = (0, 1) if u8 else (1, 2)
    out = []
    for i in range(8):
        x = img
        if i & 1:
            x = torch.flip(x, [W])
        if i & 2:
            x = torch.flip(x, [H])
        if i & 4:
            x = x.transpose(H, W)
        out.append(x)
    return torch.stack(out)


def torch_merge(outs):
    res = []
    for y in outs:                       # (8,C,T,T) each
        acc = None
        for i in range(8):
            z = y[i].float()
            if i & 4:
                z = z.transpose(-2, -1)
            if i & 2:
                z = torch.flip(z, [-2])
            if i & 1:
                z = torch.flip(z, [-1])
            acc = z if acc is None else acc + z
        res.append((acc * 0.125)[None])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--load-size", type=int, default=256, help="256 -> 512 x 512 images")
    ap.add_argument("--u8", action="store_true", help="uint8 images in, uint8 images out (test.py --u8_input); default fp32 in and out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py needs a GPU")
    dev = "cuda:0"
    cfg = NetConfig(24, 4, patch_size=args.load_size // 8, load_size=args.load_size)
    net = dec_ipt(cfg, compute_dtype=args.dtype)
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to(dev)
    net.output_f16 = args.dtype == "fp16"          # the forwards write fp16 outputs straight into the arena, as bench_tiled.py has them
    T = cfg.image_size
    g = torch.Generator().manual_seed(0)
    if args.u8:
        img = torch.randint(0, 256, (1, T, T, 3), generator=g, dtype=torch.uint8).to(dev)
    else:
        img = (torch.rand(1, 3, T, T, generator=g) * 2 - 1).to(dev)
    odt = torch.float16 if net.output_f16 else torch.float32
    esz = 2 if net.output_f16 else 4
    slab_in = ops.x8_expand(img, 0)
    arena = torch.empty(56 * T * T, dtype=odt, device=dev)
    px = 8 * T * T
    views = [arena[:3 * px].view(8, 3, T, T), arena[3 * px:4 * px].view(8, 1, T, T), arena[4 * px:].view(8, 3, T, T)]

    with torch.no_grad():
        for _ in range(3):                  # warm-up: plans, workspaces, code objects, the allocator's blocks
            net.forward_x8(img, output_u8=args.u8)
            net(slab_in, out=arena)
            ops.x8_merge(arena, 1, T, output_u8=args.u8)
            torch_merge(views)
            torch_expand(img[0], args.u8)
        torch.cuda.synchronize()
        t_x8 = timed(lambda: net.forward_x8(img, output_u8=args.u8))
        t_plain = timed(lambda: net(slab_in, out=arena))
        t_expand = timed(lambda: ops.x8_expand(img, 0, out=slab_in), inner=20)
        t_merge = timed(lambda: ops.x8_merge(arena, 1, T, output_u8=args.u8), inner=20)
        t_texp = timed(lambda: torch_expand(img[0], args.u8), inner=5)
        t_tmerge = timed(lambda: torch_merge(views), inner=5)
    in_px = 3 * T * T * (1 if args.u8 else 4)
    expand_bytes = 9 * in_px
    merge_bytes = 56 * T * T * esz + (9 * T * T if args.u8 else 7 * T * T * 4)
    res = {"what": "self-ensemble x8, one %d x %d image" % (T, T), "dtype": args.dtype, "arena": str(odt).replace("torch.", ""), "u8_in_out": bool(args.u8),
           "reps": REPS, "statistic": "median",
           "forward_x8_ms_per_image": round(t_x8, 4), "plain_batch8_forward_ms": round(t_plain, 4),
           "glue_ms_inside_forward_x8": round(t_x8 - t_plain, 4),
           "expand_us": round(t_expand * 1e3, 2), "merge_us": round(t_merge * 1e3, 2), "expand_plus_merge_us": round((t_expand + t_merge) * 1e3, 2),
           "expand_bytes": expand_bytes, "merge_bytes": merge_bytes,
           "expand_GBps": round(expand_bytes / (t_expand * 1e-3) / 1e9, 1), "merge_GBps": round(merge_bytes / (t_merge * 1e-3) / 1e9, 1),
           "merge_fraction_of_copy_rate": round(merge_bytes / (t_merge * 1e-3) / (COPY_TBPS * 1e12), 3),
           "torch_expand_us": round(t_texp * 1e3, 2), "torch_merge_us": round(t_tmerge * 1e3, 2),
           "torch_expand_plus_merge_us": round((t_texp + t_tmerge) * 1e3, 2),
           "kernel_pair_speedup_over_torch": round((t_texp + t_tmerge) / (t_expand + t_merge), 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
