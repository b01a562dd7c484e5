#!/usr/bin/env python3
"""Cost of overlapping-tile inference (tiled.py) on one large image: ms per image split into the tile forwards and gather + blend, and the
effective bandwidth of the blend kernel against the 6.29 TB/s measured copy rate of MI355X HBM.

    python tools/bench_tiled.py [--height 2160 --width 3840 --dtype fp16 --tile_batch 8 --reps 10]

The forwards write fp16 outputs straight into the tile arena (output_f16) under fp16; fp32 outputs otherwise.  Device events time each phase of
the same sequence dehaze_tiled runs; every phase is warmed up first.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from cfen_vit_dehazing_amd import ops, tiled
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict

COPY_TBPS = 6.29          # MI355X_MICROARCH.md: measured device-to-device copy rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--load-size", type=int, default=256, help="256 -> 512 x 512 tiles")
    ap.add_argument("--tile_batch", type=int, default=8)
    ap.add_argument("--overlap", type=int, default=None)
    ap.add_argument("--u8", action="store_true", help="uint8 image in, uint8 images out (test.py --u8_input); default fp32 in and out")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tiled.py needs a GPU")
    dev = "cuda:0"
    cfg = NetConfig(24, 4, patch_size=args.load_size // 8, load_size=args.load_size)
    net = dec_ipt(cfg, compute_dtype=args.dtype)
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to(dev)
    net.output_f16 = args.dtype == "fp16"
    H, W, T = args.height, args.width, cfg.image_size
    o = tiled.default_overlap(T) if args.overlap is None else args.overlap
    ys, xs = tiled.tile_grid(H, W, T, o)
    ny, nx = len(ys), len(xs)
    n = ny * nx
    B = min(args.tile_batch, n)
    nslabs = -(-n // B)
    g = torch.Generator().manual_seed(0)
    if args.u8:
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        slab_in = torch.empty(B, T, T, 3, dtype=torch.uint8, device=dev)
    else:
        img = (torch.rand(3, H, W, generator=g) * 2 - 1).to(dev)
        slab_in = torch.empty(B, 3, T, T, dtype=torch.float32, device=dev)
    odt = torch.float16 if net.output_f16 else torch.float32
    slab = 7 * B * T * T
    arena = torch.empty(nslabs * slab, dtype=odt, device=dev)

    def gather(s):
        ops.tile_gather(img, T, ny, nx, s * B, B, out=slab_in)

    def forward(s):
        net(slab_in, out=arena[s * slab:(s + 1) * slab])

    def blend():
        return ops.tile_blend(arena, B, T, H, W, ny, nx, o, output_u8=args.u8)

    with torch.no_grad():
        for s in range(nslabs):                 # warm-up: plan, workspace, code objects
            gather(s)
            forward(s)
        blend()
        torch.cuda.synchronize()
        ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
        t_gather = t_fwd = t_blend = t_total = 0.0
        for _ in range(args.reps):
            e0, e3 = ev(), ev()
            e0.record()
            for s in range(nslabs):
                a, b, c = ev(), ev(), ev()
                a.record()
                gather(s)
                b.record()
                forward(s)
                c.record()
                c.synchronize()
                t_gather += a.elapsed_time(b)
                t_fwd += b.elapsed_time(c)
            a, b = ev(), ev()
            a.record()
            blend()
            b.record()
            e3.record()
            e3.synchronize()
            t_blend += a.elapsed_time(b)
            t_total += e0.elapsed_time(e3)
        # the whole public call, back to back, no per-phase events
        for _ in range(2):
            tiled.dehaze_tiled(net, img, overlap=o, tile_batch=args.tile_batch, output_u8=args.u8)
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for _ in range(args.reps):
            tiled.dehaze_tiled(net, img, overlap=o, tile_batch=args.tile_batch, output_u8=args.u8)
        e1.record()
        e1.synchronize()
        t_call = e0.elapsed_time(e1) / args.reps
    r = args.reps
    t_gather, t_fwd, t_blend, t_total = t_gather / r, t_fwd / r, t_blend / r, t_total / r
    # bytes the blend must move: every arena slot it reads (n tiles x 7 planes) once, plus the outputs
    esz = 2 if odt == torch.float16 else 4
    read = n * 7 * T * T * esz
    written = H * W * (9 if args.u8 else 7 * 4)
    blend_tbps = (read + written) / (t_blend * 1e-3) / 1e12
    print(json.dumps({
        "image": [H, W], "tile": T, "overlap": o, "tiles": [ny, nx], "tile_batch": B, "batches": nslabs, "dtype": args.dtype,
        "arena": str(odt).replace("torch.", ""), "io": "u8" if args.u8 else "fp32",
        "ms_per_image_phased": round(t_total, 3), "ms_per_image_dehaze_tiled": round(t_call, 3),
        "ms_forwards": round(t_fwd, 3), "ms_gather": round(t_gather, 4), "ms_blend": round(t_blend, 4),
        "gather_blend_share_pct": round(100 * (t_gather + t_blend) / max(t_total, 1e-9), 2),
        "blend_bytes_MB": round((read + written) / 1e6, 1), "blend_TBps": round(blend_tbps, 3),
        "blend_share_of_copy_rate_pct": round(100 * blend_tbps / COPY_TBPS, 1)}))


if __name__ == "__main__":
    main()
