#!/usr/bin/env python3
"""Writes tests/golden/metrics_pairs.npz: what the REFERENCE's pytorch_msssim.ssim gives for the image pairs of tests/metrics_images.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_metrics.py --reference <checkout of the reference project>

A generator script: it runs on the CPU, needs the reference checkout (for `pytorch_msssim`), and is not part of any test or GPU run.  Per image of
every case the fixture holds
    ref32   the reference: pytorch_msssim.ssim(img1, img2, window_size=11, size_average=True, val_range=1) on (1,3,H,W) fp32 tensors v / 255
    f64     the float64 restatement of the same definition (metrics_images.ssim_f64_u8)
    sse     the exact integer sum of squared byte differences
    crc_a / crc_b  CRC32 of the regenerated images (they are not stored)
and `max_ref32_f64` = max |ref32 - f64| over all of them: the reference's own fp32 rounding distance, the unit of the tests' bars."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (holds pytorch_msssim/)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "metrics_pairs.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import torch
    import pytorch_msssim
    import metrics_images as mi

    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    names, offsets, ref32, f64, sse, crc_a, crc_b = [], [0], [], [], [], [], []
    for name in mi.CASES:
        a, b = mi.pair(name)
        names.append(name)
        crc_a.append(mi.crc(a))
        crc_b.append(mi.crc(b))
        for i in range(a.shape[0]):
            ta = torch.from_numpy(a[i]).permute(2, 0, 1)[None].float() / 255.0
            tb = torch.from_numpy(b[i]).permute(2, 0, 1)[None].float() / 255.0
            with torch.no_grad():
                r = float(pytorch_msssim.ssim(ta, tb, window_size=11, size_average=True, val_range=1))
            d = mi.ssim_f64_u8(a[i], b[i])
            ref32.append(r)
            f64.append(d)
            sse.append(mi.sse_int(a[i], b[i]))
            print("%-20s image %d  ref32 %.9f  f64 %.12f  |diff| %.3e  sse %d" % (name, i, r, d, abs(r - d), sse[-1]))
        offsets.append(len(ref32))
    ref32, f64 = np.array(ref32, dtype=np.float64), np.array(f64, dtype=np.float64)
    dist = float(np.abs(ref32 - f64).max())
    print("max |ref32 - f64| = %.3e" % dist)
    np.savez(args.out, names=np.array(names), offsets=np.array(offsets, dtype=np.int64), ref32=ref32, f64=f64, sse=np.array(sse, dtype=np.int64),
             crc_a=np.array(crc_a, dtype=np.uint32), crc_b=np.array(crc_b, dtype=np.uint32), max_ref32_f64=np.float64(dist))


if __name__ == "__main__":
    main()
