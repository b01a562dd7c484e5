#!/usr/bin/env python3
"""Device time of the flicker score (cfen_flicker_u8; csrc/k_flicker.hip, include/cfen_flicker.h) beside the search it follows:

    python3 tools/bench_flicker.py [out.json]         (default profiles/flicker_bench.json)

for eight 512 x 512 frames and for one 540 x 960 frame (the working resolution of a 2160 x 3840 stream), at block 16: ops.flicker_u8 with the
searched field and with the zero field, ops.motion_search_u8 at range 8 on the same frames, a device copy of the four frame sets the score
reads (12 bytes per pixel, read once; the copy also writes them), and the whole flicker.Scorer.step with one and with two targets -- which ends
in a copy of its results to the host and waits for it.  The frames are tools/bench_motion.py's panning clip.  The method is
tools/bench_motion.py's: events around 50 back-to-back calls, the median of 7 runs.  Prints the JSON object it writes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

from bench_motion import clip
from bench_temporal import DEV, timed, us
from cfen_vit_dehazing_amd import flicker, ops

D = flicker.DEFAULTS


def case(n, h, w, seed):
    G, Y = clip(n, h, w, seed, 1)
    bh, bw = -(-h // D["block"]), -(-w // D["block"])
    vec = torch.empty(n, bh, bw, 2, dtype=torch.int16, device=DEV)
    sad = torch.empty(n, bh, bw, dtype=torch.int32, device=DEV)
    sums = torch.empty(n, 8, dtype=torch.int64, device=DEV)
    res = {"case": "%d x %dx%d at the working resolution, block %d, range %d, bias %d, tol %d" % (n, h, w, D["block"], D["range"], D["bias"], D["tol"])}
    t = timed(lambda: ops.motion_search_u8(G[1:], G[0], D["block"], D["range"], D["bias"], out=(vec, sad)))
    res["motion_search_u8 (k_motion_search), %d frames" % n] = us(t)
    read = 12 * n * h * w
    for name, v in (("searched field", vec), ("zero field (vec = NULL)", None)):
        t = timed(lambda: ops.flicker_u8(G[1:], G[0], Y[1:], Y[0], v, D["block"], D["tol"], out=sums))
        res["flicker_u8 (k_flicker + k_flicker_finish), %s" % name] = dict(us(t), bytes_read=read, bytes_read_per_s=round(read / (t[0] * 1e-3), 0))
    s = sums.cpu()
    res["share of the pixels matched (zero field)"] = round(float(s[:, 1].sum()) / (n * h * w), 4)
    res["share of non-zero vectors"] = round(float((vec != 0).any(dim=3).float().mean()), 4)
    srcs = (G[1:], G[0], Y[1:], Y[0])
    dsts = tuple(torch.empty_like(t_) for t_ in srcs)

    def copy():
        for d, s_ in zip(dsts, srcs):
            d.copy_(s_)
    res["device copy of the four frame sets (4 copies)"] = dict(us(timed(copy)), bytes_read=sum(t_.numel() for t_ in srcs))
    O = (Y.int() + 1).clamp(max=255).to(torch.uint8)
    for name, out in (("Scorer.step, one target", None), ("Scorer.step, two targets", O)):
        sc = flicker.Scorer()
        sc.step(G[:1], Y[:1], None if out is None else out[:1])
        res[name + " (search, %s, one copy to the host)" % ("one flicker_u8" if out is None else "two flicker_u8")] = \
            us(timed(lambda: sc.step(G[1:], Y[1:], None if out is None else out[1:])))
    return res


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "flicker_bench.json")
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events, 50 calls per run, median of 7 runs"}
    res["8 x 512x512"] = case(8, 512, 512, 3)
    print(json.dumps(res["8 x 512x512"]), flush=True)
    res["1 x 540x960"] = case(1, 540, 960, 4)
    print(json.dumps(res["1 x 540x960"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
