"""PSNR and SSIM of dehazed images against their ground truth, computed on the device (csrc/k_metrics.hip through ops.image_metrics).

Definition (fixed; include/cfen_hip.h has the long form).  Both images are scored as values in [0,1], data range L = 1:
  SSIM  the reference's pytorch_msssim.ssim(img1, img2, window_size=11, size_average=True, val_range=1) (pytorch_msssim/__init__.py:19-70): an
        11 x 11 Gaussian window (sigma 1.5), valid convolution, C1 = 0.01^2, C2 = 0.03^2, the mean over the 3 channels and all window positions.
  PSNR  10 log10(1 / MSE), the MSE over all 3 H W values; inf for equal images.  The reference has no PSNR code: this is the standard
        definition, taken over the RGB values -- NOT over the Y channel of YCbCr some dehazing papers report.
Images under 11 x 11 are refused: the reference shrinks its window there, this project does not follow it.

CUDA tensors only; there is no CPU fallback.  `format_csv` / `summarize` are the text side of test.py --eval."""
import math

CSV_HEADER = "image,psnr,ssim"


def psnr_from_sse(sse, n_values):
    """PSNR in dB from a sum of squared errors on the 0..255 scale over n_values values: 10 log10(255^2 n / sse), inf when sse == 0"""
    if sse < 0 or n_values <= 0:
        raise ValueError("psnr_from_sse: sse %r over %r values" % (sse, n_values))
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n_values / sse)


def psnr_ssim(out, gt, value_range=(-1.0, 1.0)):
    """[(psnr, ssim), ...] per image, Python floats.  out, gt: (B,H,W,3) / (H,W,3) uint8 or (B,C,H,W) / (C,H,W) float32 CUDA tensors of equal shape;
    value_range maps float images to [0,1] (ignored for uint8).  One device pass and one copy of 16 B bytes back."""
    import torch
    from . import ops
    if not isinstance(out, torch.Tensor) or not isinstance(gt, torch.Tensor) or not out.is_cuda or not gt.is_cuda:
        raise ValueError("psnr_ssim needs CUDA tensors; there is no CPU fallback")
    sse, ssim = ops.image_metrics(out.contiguous(), gt.contiguous(), value_range=value_range)
    n = out.numel() // sse.numel()
    both = torch.stack([sse, ssim], dim=1).cpu().tolist()
    return [(psnr_from_sse(s, n), float(m)) for s, m in both]


def _fmt(v):
    return "inf" if math.isinf(v) else "%.6f" % v


def format_csv(rows):
    """the text of metrics.csv: header `image,psnr,ssim`, one row per (image, psnr, ssim) in the order given, %.6f, an infinite PSNR as `inf`"""
    return "".join([CSV_HEADER + "\n"] + ["%s,%s,%s\n" % (name, _fmt(p), _fmt(s)) for name, p, s in rows])


def summarize(rows):
    """{'images', 'psnr_mean' (over the finite values, nan when there is none), 'psnr_infinite' (how many are inf), 'ssim_mean'}"""
    finite = [p for _, p, _ in rows if math.isfinite(p)]
    return {"images": len(rows),
            "psnr_mean": sum(finite) / len(finite) if finite else float("nan"),
            "psnr_infinite": sum(1 for _, p, _ in rows if math.isinf(p)),
            "ssim_mean": sum(s for _, _, s in rows) / len(rows) if rows else float("nan")}


def summary_line(rows):
    s = summarize(rows)
    return "eval: %d images, mean PSNR %.4f dB over %d finite (%d infinite), mean SSIM %.6f" % (
        s["images"], s["psnr_mean"], s["images"] - s["psnr_infinite"], s["psnr_infinite"], s["ssim_mean"])
