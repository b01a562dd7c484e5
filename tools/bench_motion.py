#!/usr/bin/env python3
"""Device time of motion compensation (cfen_motion_search_u8 + cfen_motion_warp; csrc/k_motion.hip, include/cfen_motion.h), and what it adds to
Stabiliser.step:

    python3 tools/bench_motion.py [out.json]         (default profiles/motion_bench.json)

for eight 512 x 512 frames (down = auto = 1) and for one 2160 x 3840 frame (down = auto = 4: 540 x 960): ops.motion_search_u8 on the batch and
ops.motion_warp on one frame at block 16, range 8, and the whole Stabiliser.step without and with mc_range = 8, in the same session.  The frames
are a window panning (2, 5) working-resolution pixels per frame over a noisy picture, so the vectors are not zero.  The method is
tools/bench_temporal.py's: events around 50 back-to-back calls, the median of 7 runs.  Pixel differences formed by the search and their rate,
and the dword LDS reads of the inner loop (one per pixel and candidate) as bytes per second.  Prints the JSON object it writes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_temporal import DEV, timed, us
from cfen_vit_dehazing_amd import ops, temporal

BLOCK, RANGE = 16, 8


def clip(n, H, W, seed, scale):
    """n + 1 frames (H, W, 3) uint8 of a window that moves (2, 5) * scale pixels per frame over a smooth-plus-noise picture, and 'dehazed' ones"""
    rs = np.random.RandomState(seed)
    dy, dx = 2 * scale, 5 * scale
    yy, xx = np.mgrid[0:H + dy * n, 0:W + dx * n].astype(np.float32)
    big = np.stack([np.sin(xx / 37 + yy / 53) * 70 + 128, np.cos(yy / 29 - xx / 61) * 60 + 120, (xx + yy) / (H + W) * 100 + 60], -1)
    big = np.clip(big + rs.randn(*big.shape).astype(np.float32) * 10, 0, 255).astype(np.uint8)
    G = np.stack([big[dy * k:dy * k + H, dx * k:dx * k + W] for k in range(n + 1)])
    Y = np.clip(G * 0.8 + 20 + rs.randn(n + 1, 1, 1, 3) * 5, 0, 255).astype(np.uint8)
    return torch.from_numpy(G).to(DEV), torch.from_numpy(Y).to(DEV)


def case(n, H, W, seed):
    S, h, w = temporal.working_size(H, W)
    G, Y = clip(n, H, W, seed, S)
    I = G if S == 1 else ops.resample_u8(G, (h, w), filter="box")
    bh, bw = -(-h // BLOCK), -(-w // BLOCK)
    vec = torch.empty(n, bh, bw, 2, dtype=torch.int16, device=DEV)
    sad = torch.empty(n, bh, bw, dtype=torch.int32, device=DEV)
    state = torch.randn(h, w, 6, device=DEV)
    outs = (torch.empty(h, w, 3, dtype=torch.uint8, device=DEV), torch.empty(h, w, 6, device=DEV))
    res = {"case": "%d x %dx%d, working resolution %dx%d (down = auto = %d), block %d, range %d, bias %d"
                   % (n, H, W, h, w, S, BLOCK, RANGE, temporal.MC_DEFAULTS["bias"])}
    t = timed(lambda: ops.motion_search_u8(I[1:], I[0], BLOCK, RANGE, temporal.MC_DEFAULTS["bias"], out=(vec, sad)))
    diffs = n * h * w * (2 * RANGE + 1) ** 2
    res["motion_search_u8 (k_motion_search), %d frames" % n] = dict(
        us(t), blocks=n * bh * bw, pixel_differences=diffs, pixel_differences_per_s=round(diffs / (t[0] * 1e-3), 0),
        lds_read_bytes_inner_loop=4 * diffs, lds_read_bytes_per_s=round(4 * diffs / (t[0] * 1e-3), 0))
    res["share of non-zero vectors"] = round(float((vec != 0).any(dim=3).float().mean()), 4)
    t = timed(lambda: ops.motion_warp(vec[0], I[0], state, BLOCK, out=outs))
    res["motion_warp (k_motion_warp), one frame"] = dict(us(t), bytes_moved=2 * h * w * 27, bytes_per_s=round(2 * h * w * 27 / (t[0] * 1e-3), 0))
    out = torch.empty_like(G[1:])
    for name, kw in (("Stabiliser.step without compensation", {}), ("Stabiliser.step with mc_range = %d" % RANGE, {"mc_range": RANGE, "mc_block": BLOCK})):
        st = temporal.Stabiliser(**kw)
        st.step(G[:1], Y[:1])
        res[name] = us(timed(lambda: st.step(G[1:], Y[1:], out=out)))
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "motion_bench.json")
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events, 50 calls per run, median of 7 runs"}
    res["8 x 512x512"] = case(8, 512, 512, 3)
    print(json.dumps(res["8 x 512x512"]), flush=True)
    res["1 x 2160x3840"] = case(1, 2160, 3840, 4)
    print(json.dumps(res["1 x 2160x3840"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
