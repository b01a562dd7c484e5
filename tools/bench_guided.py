#!/usr/bin/env python3
"""Device time of guided upsampling (cfen_guided_coef_u8 + cfen_guided_apply_u8; csrc/k_guided.hip, include/cfen_guided.h) beside the bicubic
resample it replaces, and of fit-to-size inference with and without it:

    python3 tools/bench_guided.py [out.json] [--ops-only]         (default profiles/guided_bench.json)
    python3 tools/bench_guided.py --fold-trace kernel_trace.csv out.json

guided    2160 x 3840 from 512 x 512, B = 1, radius 2: ops.guided_upsample_u8 and its two halves -- guided_coef_u8 (k_guided_coef and
          k_guided_mean together: they share one entry point, and events cannot look inside it) and guided_apply_u8 (k_guided_apply) -- beside
          ops.resample_u8 of the same output, the call it replaces: events around `reps` back-to-back calls, the median of 7 runs.  The apply
          kernel's bytes (guide read + output written + coefficients read once) and their rate as a share of the 6.29 TB/s copy rate DESIGN uses.
fit       net.forward_fit of a 2160 x 3840 image (fp16, u8 input) with refine=None and refine="guided".
          --ops-only leaves this part out: the run to put under `rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own,
          which times the three kernels apart.  --fold-trace turns that run's kernel trace into the median per kernel (k_guided_coef and
          k_guided_mean apart for the calls at radius 2 and at radius 16, told apart by their duration) -> profiles/guided_kernel_split.json;
          the run's own statistics file is profiles/guided_kernel_stats.csv.
Prints the JSON object it writes."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cfen_vit_dehazing_amd import ops
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


def us(t):
    return {"device_us": round(t[0] * 1e3, 2), "device_us_min_max": [round(t[1] * 1e3, 2), round(t[2] * 1e3, 2)]}


def fold_trace(trace_csv, out_path):
    """rocprofv3's kernel trace of an --ops-only run -> median duration per kernel.  That run calls the two low-resolution kernels at radius 2 and
    at radius 16; the two groups are an order of magnitude apart in time and are split at the largest gap between sorted durations"""
    import csv
    times = {}
    for row in csv.DictReader(open(trace_csv)):
        for k in ("k_guided_coef", "k_guided_mean", "k_guided_apply"):
            if k in row["Kernel_Name"]:
                times.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res = {"source": "rocprofv3 --kernel-trace --stats of `tools/bench_guided.py --ops-only` (2160 x 3840 from 512 x 512, B = 1), a run of its own", "unit": "us"}
    for k, v in times.items():
        v.sort()
        if k == "k_guided_apply":
            res[k] = {"calls": len(v), "median": round(statistics.median(v), 2), "min_max": [round(v[0], 2), round(v[-1], 2)]}
            continue
        cut = max(range(1, len(v)), key=lambda i: v[i] - v[i - 1])
        res[k] = {name: {"calls": len(g), "median": round(statistics.median(g), 2), "min_max": [round(g[0], 2), round(g[-1], 2)]}
                  for name, g in (("radius_2", v[:cut]), ("radius_16", v[cut:]))}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


def main():
    if "--fold-trace" in sys.argv:
        i = sys.argv.index("--fold-trace")
        return fold_trace(sys.argv[i + 1], sys.argv[i + 2])
    args = [a for a in sys.argv[1:] if a != "--ops-only"]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "guided_bench.json")
    H, W, T, r = 2160, 3840, 512, 2
    rs = np.random.RandomState(3)
    G = torch.from_numpy(rs.randint(0, 256, (1, H, W, 3), dtype=np.uint8)).to(DEV)
    I = ops.resample_u8(G, (T, T))
    P = torch.from_numpy(rs.randint(0, 256, (1, T, T, 3), dtype=np.uint8)).to(DEV)
    out = torch.empty(1, H, W, 3, dtype=torch.uint8, device=DEV)
    coef = ops.guided_coef_u8(I, P, r)
    res = {"device": torch.cuda.get_device_name(0), "case": "1 x %dx%d -> %dx%d, radius %d" % (T, T, H, W, r),
           "timing": "device events, 20 calls per run, median of 7 runs"}
    res["guided_upsample_u8"] = us(timed(lambda: ops.guided_upsample_u8(G, I, P, r, out=out)))
    res["guided_coef_u8 (k_guided_coef + k_guided_mean)"] = us(timed(lambda: ops.guided_coef_u8(I, P, r, out=coef)))
    res["guided_coef_u8 at radius 16"] = us(timed(lambda: ops.guided_coef_u8(I, P, 16)))
    apply_t = timed(lambda: ops.guided_apply_u8(coef, G, out=out))
    moved = 2 * H * W * 3 + T * T * 24
    res["guided_apply_u8 (k_guided_apply)"] = dict(us(apply_t), bytes_moved=moved, share_of_copy_rate=round(moved / (apply_t[0] * 1e-3) / COPY_RATE, 4))
    res["resample_u8 bicubic, the call it replaces"] = us(timed(lambda: ops.resample_u8(P, (H, W), out=out)))
    print(json.dumps(res), flush=True)
    if "--ops-only" in sys.argv:
        return
    cfg = NetConfig(24, 4, patch_size=32, load_size=256)          # T = 512, the shipped configuration
    net = dec_ipt(cfg, compute_dtype="fp16")
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to(DEV)
    plain = timed(lambda: net.forward_fit(G), reps=5)
    guided = timed(lambda: net.forward_fit(G, refine="guided"), reps=5)
    res["fit_2160x3840"] = {"forward_fit_ms": round(plain[0], 3), "forward_fit_ms_min_max": [round(plain[1], 3), round(plain[2], 3)],
                            "forward_fit_guided_ms": round(guided[0], 3), "forward_fit_guided_ms_min_max": [round(guided[1], 3), round(guided[2], 3)],
                            "note": "fp16, uint8 input and outputs; forward_fit = resample + one batch-1 forward + three resamples back; "
                                    "refine='guided' replaces the third resample by guided_upsample_u8"}
    print(json.dumps(res["fit_2160x3840"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
