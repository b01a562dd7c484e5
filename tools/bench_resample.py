#!/usr/bin/env python3
"""Device time of the PIL-exact uint8 resampling (cfen_resample_u8; cfen_vit_dehazing_amd/resample.py, csrc/k_resample.hip) beside PIL on one host
thread, and of fit-to-size inference beside tiled inference of the same image:

    python3 tools/bench_resample.py [out.json]          (default profiles/resample_bench.json)

resample  2160 x 3840 -> 512 x 512 and back (B = 1, and B = 3: the three outputs), eight 460 x 620 <-> 512 x 512: events around `reps` back-to-back
          calls, the median of 7 runs; bytes moved = source + destination + twice the uint8 intermediate, and their rate as a share of the
          6.29 TB/s copy rate DESIGN uses.  PIL's Image.resize of the same arrays on one thread, median of 7.
fit       net.forward_fit of a 2160 x 3840 image (fp16, u8 input) beside tiled.dehaze_tiled of the same image (17.3 ms).
Prints the JSON object it writes."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

from cfen_vit_dehazing_amd import ops, tiled
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict

DEV = "cuda:0"
COPY_RATE = 6.29e12          # bytes / s, the device copy rate of DESIGN section 6


def timed(fn, reps=20, runs=7):
    """median over `runs` of the time per call in ms of `reps` back-to-back calls between two events"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def resample_case(B, src, dst, filter="bicubic"):
    (H, W), (H2, W2) = src, dst
    a = np.random.RandomState(B * H + W2).randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    t = torch.from_numpy(a).to(DEV)
    out = torch.empty(B, H2, W2, 3, dtype=torch.uint8, device=DEV)
    med, lo, hi = timed(lambda: ops.resample_u8(t, (H2, W2), filter, out=out))
    moved = B * 3 * (H * W + (2 * H * W2 if (H != H2 and W != W2) else 0) + H2 * W2)
    host = []
    imgs = [Image.fromarray(x) for x in a]
    for _ in range(7):
        t0 = time.perf_counter()
        for im in imgs:
            im.resize((W2, H2), Image.BICUBIC)
        host.append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(np.asarray(im.resize((W2, H2), Image.BICUBIC)), o) for im, o in zip(imgs, out.cpu().numpy()))
    return {"case": "%d x %dx%d -> %dx%d" % (B, H, W, H2, W2), "device_us": round(med * 1e3, 2), "device_us_min_max": [round(lo * 1e3, 2), round(hi * 1e3, 2)],
            "bytes_moved": moved, "share_of_copy_rate": round(moved / (med * 1e-3) / COPY_RATE, 4), "pil_one_thread_ms": round(statistics.median(host), 3),
            "equals_pil": bool(same)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "resample_bench.json")
    res = {"device": torch.cuda.get_device_name(0), "filter": "bicubic", "timing": "device events, 20 calls per run, median of 7 runs", "resample": []}
    for B, src, dst in ((1, (2160, 3840), (512, 512)), (1, (512, 512), (2160, 3840)), (3, (512, 512), (2160, 3840)),
                        (8, (460, 620), (512, 512)), (8, (512, 512), (460, 620))):
        res["resample"].append(resample_case(B, src, dst))
        print(json.dumps(res["resample"][-1]), flush=True)
    cfg = NetConfig(24, 4, patch_size=32, load_size=256)          # T = 512, the shipped configuration
    net = dec_ipt(cfg, compute_dtype="fp16")
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to(DEV)
    img = torch.from_numpy(np.random.RandomState(7).randint(0, 256, (2160, 3840, 3), dtype=np.uint8)).to(DEV)
    fit = timed(lambda: net.forward_fit(img[None]), reps=5)
    til = timed(lambda: tiled.dehaze_tiled(net, img, output_u8=True), reps=3)
    res["fit_2160x3840"] = {"forward_fit_ms": round(fit[0], 3), "forward_fit_ms_min_max": [round(fit[1], 3), round(fit[2], 3)],
                            "dehaze_tiled_ms": round(til[0], 3), "dehaze_tiled_ms_min_max": [round(til[1], 3), round(til[2], 3)],
                            "note": "fp16, uint8 input and outputs; forward_fit = resample + one batch-1 forward + three resamples back; "
                                    "dehaze_tiled = 45 tiles in six batch-8 forwards + blend"}
    print(json.dumps(res["fit_2160x3840"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
