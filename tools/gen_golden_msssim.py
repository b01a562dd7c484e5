#!/usr/bin/env python3
"""Writes tests/golden/msssim_pairs.npz: what the REFERENCE's pytorch_msssim.msssim gives for the image pairs of tests/msssim_ref.py.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_msssim.py --reference <checkout of the reference project>

A generator script: it runs on the CPU, needs the reference checkout (for `pytorch_msssim`, imported from where it lies; nothing of it is copied),
and is not part of any test or GPU run.  Per image of every case the fixture holds
    ref32_ms      the reference: pytorch_msssim.msssim(img1, img2, window_size=11, size_average=True, val_range=1, normalize=None) on (1,3,H,W)
                  fp32 tensors v / 255 (NaN where a used term is negative)
    ref32_levels  (5, 2): the reference's (ssim_l, cs_l) = pytorch_msssim.ssim(..., full=True) on its own F.avg_pool2d images
    f64_levels / f64_ms   the float64 restatement of the same definition (msssim_ref.levels_f64_u8, msssim_ref.combine)
    sse           the exact integer sum of squared byte differences
    crc_a / crc_b CRC32 of the regenerated images (they are not stored)
    D_level_pair / D_ms_pair   max |ref32 - f64| over the pair's ten level values / of its combined value (NaN where that is NaN)
and the units of the tests' bars, the reference's own fp32 rounding distances: D_level = max D_level_pair and D_ms = max D_ms_pair over the pairs
with a finite MS-SSIM, D_level_nan = the same over the others (the anticorrelated pair: its cs_l sit near -1 over small denominators and the
reference's own rounding is ten times larger there, so that pair is measured against its own distance and does not loosen the bar of the rest)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "msssim_pairs.npz"))
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import torch
    import torch.nn.functional as F
    import pytorch_msssim
    import metrics_images as mi
    import msssim_ref as mr

    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    names, offsets, ref_ms, ref_lv, f64_ms, f64_lv, sse, crc_a, crc_b = [], [0], [], [], [], [], [], [], []
    for name in mr.CASES:
        a, b = mr.pair(name)
        names.append(name)
        crc_a.append(mi.crc(a))
        crc_b.append(mi.crc(b))
        for i in range(a.shape[0]):
            ta = torch.from_numpy(a[i]).permute(2, 0, 1)[None].float() / 255.0
            tb = torch.from_numpy(b[i]).permute(2, 0, 1)[None].float() / 255.0
            with torch.no_grad():
                r = float(pytorch_msssim.msssim(ta, tb, window_size=11, size_average=True, val_range=1, normalize=None))
                lv = []
                for _ in range(mr.LEVELS):
                    s, c = pytorch_msssim.ssim(ta, tb, window_size=11, size_average=True, full=True, val_range=1)
                    lv.append((float(s), float(c)))
                    ta, tb = F.avg_pool2d(ta, (2, 2)), F.avg_pool2d(tb, (2, 2))
            d_lv = mr.levels_f64_u8(a[i], b[i])
            d = mr.combine(d_lv)
            ref_ms.append(r)
            ref_lv.append(lv)
            f64_ms.append(d)
            f64_lv.append(d_lv)
            sse.append(mi.sse_int(a[i], b[i]))
            print("%-20s image %d  ref32 %.9f  f64 %.12f  |diff| %.3e  min cs %.6f  max level |diff| %.3e"
                  % (name, i, r, d, abs(r - d), d_lv[:, 1].min(), np.abs(np.array(lv) - d_lv).max()))
        offsets.append(len(ref_ms))
    ref_ms, f64_ms = np.array(ref_ms, dtype=np.float64), np.array(f64_ms, dtype=np.float64)
    ref_lv, f64_lv = np.array(ref_lv, dtype=np.float64), np.array(f64_lv, dtype=np.float64)
    # the anticorrelated pair must really take the NaN path: a negative used term, NaN from both, every level value finite
    k = names.index("anticorrelated_176")
    j = offsets[k]
    assert min(f64_lv[j, :4, 1].min(), f64_lv[j, 4, 0]) < 0 and np.isnan(ref_ms[j]) and np.isnan(f64_ms[j]), "anticorrelated_176 has no negative level"
    assert np.isfinite(ref_lv).all() and np.isfinite(f64_lv).all()
    finite = np.isfinite(f64_ms)
    assert (np.isfinite(ref_ms) == finite).all() and finite.sum() == len(f64_ms) - 1
    d_level_pair = np.abs(ref_lv - f64_lv).reshape(len(f64_ms), -1).max(axis=1)
    d_ms_pair = np.abs(ref_ms - f64_ms)
    d_level, d_level_nan, d_ms = float(d_level_pair[finite].max()), float(d_level_pair[~finite].max()), float(d_ms_pair[finite].max())
    print("D_level = %.3e   D_level_nan = %.3e   D_ms = %.3e" % (d_level, d_level_nan, d_ms))
    np.savez(args.out, names=np.array(names), offsets=np.array(offsets, dtype=np.int64), ref32_ms=ref_ms, ref32_levels=ref_lv, f64_ms=f64_ms,
             f64_levels=f64_lv, sse=np.array(sse, dtype=np.int64), crc_a=np.array(crc_a, dtype=np.uint32), crc_b=np.array(crc_b, dtype=np.uint32),
             D_level_pair=d_level_pair, D_ms_pair=d_ms_pair, D_level=np.float64(d_level), D_level_nan=np.float64(d_level_nan), D_ms=np.float64(d_ms))


if __name__ == "__main__":
    main()
