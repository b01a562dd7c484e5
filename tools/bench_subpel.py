#!/usr/bin/env python3
"""Device time of the sub-pixel refinement and warp (cfen_motion_refine_u8 + cfen_motion_warp_subpel; csrc/k_subpel.hip, include/cfen_subpel.h),
beside the whole-pixel search and warp on the same inputs, and what they add to Stabiliser.step:

    python3 tools/bench_subpel.py [out.json]         (default profiles/subpel_bench.json)

for eight 512 x 512 frames (down = auto = 1) and for one 2160 x 3840 frame (down = auto = 4: 540 x 960): ops.motion_search_u8 at range 8,
ops.motion_refine_u8 at 1/2 and 1/4 pixel on its vectors, ops.motion_warp and ops.motion_warp_subpel on one frame, all at block 16, and the whole
Stabiliser.step at mc_subpel 1, 2 and 4, in the same session.  The frames are tools/bench_motion.py's panning picture, rendered on a grid of
quarter working-resolution pixels and box-reduced, under a window that moves (2.5, 5.25) working-resolution pixels per frame, so the vectors
are fractional.  The method is tools/bench_motion.py's: events around 50 back-to-back calls, the median of 7 runs.  Bilinear samples formed by
the refinement (pixels x candidates) and their rate beside the search's pixel differences; the ratio of the two kernels' times.  Prints the
JSON object it writes."""
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
STEP4 = (10, 21)             # quarter working-resolution pixels per frame: (2.5, 5.25) pixels


def clip(n, H, W, seed, S):
    """n + 1 frames (H, W, 3) uint8 of a window that moves STEP4 / 4 working-resolution pixels per frame over tools/bench_motion.py's
    smooth-plus-noise picture, and 'dehazed' ones.  S: full-resolution pixels per working-resolution pixel; the picture is rendered U = 4 / S
    (at least 1) times finer than the frame, so that a quarter of a working pixel is a whole number q of its pixels, and box-reduced by U"""
    rs = np.random.RandomState(seed)
    U = max(1, 4 // S)
    q = S * U // 4
    dy, dx = STEP4[0] * q, STEP4[1] * q
    yy, xx = np.mgrid[0:H * U + dy * n, 0:W * U + dx * n].astype(np.float32) / U
    big = np.stack([np.sin(xx / 37 + yy / 53) * 70 + 128, np.cos(yy / 29 - xx / 61) * 60 + 120, (xx + yy) / (H + W) * 100 + 60], -1)
    big = np.clip(big + rs.randn(*big.shape).astype(np.float32) * 10, 0, 255)
    G = np.stack([big[dy * k:dy * k + H * U, dx * k:dx * k + W * U].reshape(H, U, W, U, 3).mean(axis=(1, 3)) for k in range(n + 1)])
    G = np.floor(G + 0.5).astype(np.uint8)
    Y = np.clip(G * 0.8 + 20 + rs.randn(n + 1, 1, 1, 3) * 5, 0, 255).astype(np.uint8)
    return torch.from_numpy(G).to(DEV), torch.from_numpy(Y).to(DEV)


def case(n, H, W, seed):
    S, h, w = temporal.working_size(H, W)
    bias = temporal.MC_DEFAULTS["bias"]
    G, Y = clip(n, H, W, seed, S)
    I = G if S == 1 else ops.resample_u8(G, (h, w), filter="box")
    bh, bw = -(-h // BLOCK), -(-w // BLOCK)
    vec, vec4 = (torch.empty(n, bh, bw, 2, dtype=torch.int16, device=DEV) for _ in range(2))
    sad, sad4 = (torch.empty(n, bh, bw, dtype=torch.int32, device=DEV) for _ in range(2))
    state = torch.randn(h, w, 6, device=DEV)
    outs = (torch.empty(h, w, 3, dtype=torch.uint8, device=DEV), torch.empty(h, w, 6, device=DEV))
    res = {"case": "%d x %dx%d, working resolution %dx%d (down = auto = %d), block %d, range %d, bias %d, pan (%.2f, %.2f) working pixels per frame"
                   % (n, H, W, h, w, S, BLOCK, RANGE, bias, STEP4[0] / 4, STEP4[1] / 4)}
    t_search = timed(lambda: ops.motion_search_u8(I[1:], I[0], BLOCK, RANGE, bias, out=(vec, sad)))
    diffs = n * h * w * (2 * RANGE + 1) ** 2
    res["motion_search_u8 (k_motion_search), %d frames" % n] = dict(us(t_search), blocks=n * bh * bw, pixel_differences=diffs,
                                                                    pixel_differences_per_s=round(diffs / (t_search[0] * 1e-3), 0))
    for Q in (2, 4):
        t = timed(lambda: ops.motion_refine_u8(I[1:], I[0], vec, BLOCK, Q, bias, out=(vec4, sad4)))
        samples = n * h * w * (2 * Q - 1) ** 2
        res["motion_refine_u8 (k_subpel_refine), 1/%d pixel, %d frames" % (Q, n)] = dict(
            us(t), blocks=n * bh * bw, bilinear_samples=samples, bilinear_samples_per_s=round(samples / (t[0] * 1e-3), 0),
            time_over_search=round(t[0] / t_search[0], 3), share_of_fractional_vectors=round(float(((vec4 & 3) != 0).any(dim=3).float().mean()), 4),
            sad4_over_sad=round(float(sad4.sum()) / max(float(sad.sum()), 1.0), 4))
    t_warp = timed(lambda: ops.motion_warp(vec[0], I[0], state, BLOCK, out=outs))
    res["motion_warp (k_motion_warp), one frame"] = dict(us(t_warp), bytes_moved=2 * h * w * 27, bytes_per_s=round(2 * h * w * 27 / (t_warp[0] * 1e-3), 0))
    t = timed(lambda: ops.motion_warp_subpel(vec4[0], I[0], state, BLOCK, out=outs))
    res["motion_warp_subpel (k_subpel_warp), one frame"] = dict(us(t), bytes_written=h * w * 27, bytes_read_at_most=4 * h * w * 27,
                                                               time_over_warp=round(t[0] / t_warp[0], 3))
    out = torch.empty_like(G[1:])
    for Q in temporal.MC_SUBPEL:
        st = temporal.Stabiliser(mc_range=RANGE, mc_block=BLOCK, mc_subpel=Q)
        st.step(G[:1], Y[:1])
        res["Stabiliser.step with mc_range = %d, mc_subpel = %d" % (RANGE, Q)] = us(timed(lambda: st.step(G[1:], Y[1:], out=out)))
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "subpel_bench.json")
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
