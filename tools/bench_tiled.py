#!/usr/bin/env python3
"""Cost of overlapping-tile inference (tiled.py) on one large image: ms per image split into the tile forwards and gather + blend, and the
effective bandwidth of the blend kernel against the 6.29 TB/s measured copy rate of MI355X HBM.

    python tools/bench_tiled.py [--height 2160 --width 3840 --dtype fp16 --tile_batch 8 --reps 10]

The forwards write fp16 outputs straight into the tile arena (output_f16) under fp16; fp32 outputs otherwise.  Device events time each phase of
the same sequence dehaze_tiled runs; every phase is warmed up first.  Prints one JSON line.

    python tools/bench_tiled.py --pack [--count 16 --height 460 --width 620 --u8]

--pack compares, for --count copies of the image, one dehaze_tiled call per image with one dehaze_tiled_many call over all of them (tiles of
several images packed into full batches): ms per image of both public calls (device events around each call, the two paths alternating, the
median of --reps repetitions), the forwards each runs, and the time of its gather and blend launches alone (the same launches on the same
buffers, median of --reps).
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


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def bench_pack(net, args, H, W, T, o, dev):
    g = torch.Generator().manual_seed(0)
    if args.u8:
        imgs = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(args.count)]
    else:
        imgs = [(torch.rand(3, H, W, generator=g) * 2 - 1).to(dev) for _ in range(args.count)]
    odt = torch.float16 if net.output_f16 else torch.float32
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731

    def timed(fn):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def call_unpacked():
        for im in imgs:
            tiled.dehaze_tiled(net, im, overlap=o, tile_batch=args.tile_batch, output_u8=args.u8)

    def call_packed():
        tiled.dehaze_tiled_many(net, imgs, overlap=o, tile_batch=args.tile_batch, output_u8=args.u8)

    # the gather and blend launches of a path, on buffers of its own: `groups` = the images that share an arena (one each, or all)
    def phases(groups):
        state = []
        for first, last in groups:
            plan = tiled.pack_plan([(H, W)] * (last - first), T, o, args.tile_batch)
            slab = 7 * plan.B * T * T
            arena = torch.zeros(plan.nslabs * slab, dtype=odt, device=dev)
            slab_in = torch.empty((plan.B, T, T, 3) if args.u8 else (plan.B, 3, T, T), dtype=imgs[0].dtype, device=dev)
            state.append((first, plan, slab, arena, slab_in))

        def gathers():
            for first, plan, slab, arena, slab_in in state:
                for segs in plan.slabs:
                    for k, t0, count, lane in segs:
                        ops.tile_gather(imgs[first + k], T, plan.images[k][1], plan.images[k][2], t0, count, out=slab_in[lane:lane + count])

        def blends():
            for first, plan, slab, arena, slab_in in state:
                for k, (slot0, ny, nx) in enumerate(plan.images):
                    ops.tile_blend(arena[(slot0 // plan.B) * slab:], plan.B, T, H, W, ny, nx, o, output_u8=args.u8, lane0=slot0 % plan.B)

        forwards = sum(plan.nslabs for _, plan, _, _, _ in state)
        slots = sum(plan.nslabs * plan.B for _, plan, _, _, _ in state)
        launches = sum(len(segs) for _, plan, _, _, _ in state for segs in plan.slabs)
        return gathers, blends, forwards, slots, launches, state[0][1].B

    paths = {"unpacked": (call_unpacked,) + phases([(k, k + 1) for k in range(args.count)]),
             "packed": (call_packed,) + phases([(0, args.count)])}
    times = {name: {"call": [], "gather": [], "blend": []} for name in paths}
    with torch.no_grad():
        for name, (call, gathers, blends, *_rest) in paths.items():          # warm-up: plans, workspaces, code objects of every shape in play
            for _ in range(2):
                call()
                gathers()
                blends()
        torch.cuda.synchronize()
        for _ in range(args.reps):                                            # the two paths alternate inside every repetition
            for name, (call, gathers, blends, *_rest) in paths.items():
                times[name]["call"].append(timed(call))
            for name, (call, gathers, blends, *_rest) in paths.items():
                times[name]["gather"].append(timed(gathers))
                times[name]["blend"].append(timed(blends))
    ny, nx = (len(v) for v in tiled.tile_grid(H, W, T, o))
    res = {"image": [H, W], "count": args.count, "tile": T, "overlap": o, "tiles_per_image": ny * nx, "tile_batch": args.tile_batch,
           "dtype": args.dtype, "arena": str(odt).replace("torch.", ""), "io": "u8" if args.u8 else "fp32", "reps": args.reps}
    for name, (call, gathers, blends, forwards, slots, launches, B) in paths.items():
        t = times[name]
        res[name] = {"forwards": forwards, "batch": B, "slots": slots, "gather_launches": launches, "blend_launches": args.count,
                     "ms_per_image": round(_median(t["call"]) / args.count, 4), "ms_total": round(_median(t["call"]), 3),
                     "ms_total_min_max": [round(min(t["call"]), 3), round(max(t["call"]), 3)],
                     "ms_gather": round(_median(t["gather"]), 4), "ms_blend": round(_median(t["blend"]), 4),
                     "ms_gather_blend": round(_median(t["gather"]) + _median(t["blend"]), 4)}
    res["speedup"] = round(res["unpacked"]["ms_total"] / res["packed"]["ms_total"], 3)
    return res


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
    ap.add_argument("--pack", action="store_true", help="compare per-image dehaze_tiled with one packed dehaze_tiled_many over --count images")
    ap.add_argument("--count", type=int, default=16, help="--pack: number of images in the group")
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
    if args.pack:
        print(json.dumps(bench_pack(net, args, H, W, T, o, dev)))
        return
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
