"""PSNR and SSIM of dehazed images against their ground truth, computed on the device (csrc/k_metrics.hip through ops.image_metrics).

Definition (fixed; include/cfen_hip.h has the long form).  Both images are scored as values in [0,1], data range L = 1:
  SSIM  the reference's pytorch_msssim.ssim(img1, img2, window_size=11, size_average=True, val_range=1) (pytorch_msssim/__init__.py:19-70): an
        11 x 11 Gaussian window (sigma 1.5), valid convolution, C1 = 0.01^2, C2 = 0.03^2, the mean over the 3 channels and all window positions.
  PSNR  10 log10(1 / MSE), the MSE over all 3 H W values; inf for equal images.  The reference has no PSNR code: this is the standard
        definition, taken over the RGB values -- NOT over the Y channel of YCbCr some dehazing papers report.
  MS-SSIM  the reference's pytorch_msssim.msssim(window_size=11, size_average=True, val_range=1, normalize=None) (pytorch_msssim/__init__.py:73-107):
        five levels of 2 x 2 means, at each the mean SSIM and the mean cs = (2 sigma12 + C2) / (sigma1^2 + sigma2^2 + C2) from the device
        (ops.image_msssim), then prod_{l<4} cs_l^w_l * ssim_4^w_4 here in float64; NaN when one of those five terms is negative, as in the reference.
  CIEDE2000  the mean over the pixels of the colour difference dE00 (Sharma, Wu and Dalal 2005, kL = kC = kH = 1) between the two images read as
        8-bit sRGB: bytes -> linear light by a 256-entry table -> XYZ at the matrix's own white -> Lab, a pixel with R = G = B achromatic by
        definition (include/cfen_colordiff.h has the long form).  uint8 images only; its own flag --eval_ciede2000, not a name of --eval_metrics.
Images under 11 x 11 (MS-SSIM: under 176 x 176) are refused: the reference shrinks its window there, this project does not follow it.

CUDA tensors only; there is no CPU fallback.  `format_csv` / `summarize` are the text side of test.py --eval.

Without ground truth (test.py --eval_noref, at the end of this file): statistics of the hazy input and of the dehazed output side by side, from
ops.image_noref (csrc/k_noref.hip; include/cfen_noref.h has the long form)."""
import math

CSV_HEADER = "image,psnr,ssim"
COLUMNS = ("psnr", "ssim", "msssim")                                 # what --eval_metrics may name, in the order of the csv
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
CIEDE_COLUMN = "ciede2000"                                           # --eval_ciede2000: the csv's last column, after what --eval_metrics selected
MSSSIM_MIN_EDGE = 176                                                # 11 * 2^4: the fifth level still holds one window


def psnr_from_sse(sse, n_values):
    """PSNR in dB from a sum of squared errors on the 0..255 scale over n_values values: 10 log10(255^2 n / sse), inf when sse == 0"""
    if sse < 0 or n_values <= 0:
        raise ValueError("psnr_from_sse: sse %r over %r values" % (sse, n_values))
    return float("inf") if sse == 0 else 10.0 * math.log10(255.0 ** 2 * n_values / sse)


def _need_cuda(what, *tensors):
    import torch
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
        raise ValueError("%s needs CUDA tensors; there is no CPU fallback" % what)


def psnr_ssim(out, gt, value_range=(-1.0, 1.0)):
    """[(psnr, ssim), ...] per image, Python floats.  out, gt: (B,H,W,3) / (H,W,3) uint8 or (B,C,H,W) / (C,H,W) float32 CUDA tensors of equal shape;
    value_range maps float images to [0,1] (ignored for uint8).  One device pass and one copy of 16 B bytes back."""
    import torch
    from . import ops
    _need_cuda("psnr_ssim", out, gt)
    sse, ssim = ops.image_metrics(out.contiguous(), gt.contiguous(), value_range=value_range)
    n = out.numel() // sse.numel()
    both = torch.stack([sse, ssim], dim=1).cpu().tolist()
    return [(psnr_from_sse(s, n), float(m)) for s, m in both]


def msssim_from_levels(levels):
    """MS-SSIM per image from the level values (ssim_l, cs_l): levels (B,5,2) or (5,2), a tensor (copied to the host), array or nested list.  Float64
    on the host: cs_0^w_0 cs_1^w_1 cs_2^w_2 cs_3^w_3 ssim_4^w_4, NaN when one of these five terms is negative or NaN.  A list of B floats (one float
    for a (5,2) input)."""
    if hasattr(levels, "detach"):
        levels = levels.detach().cpu()
    levels = levels.tolist() if hasattr(levels, "tolist") else levels
    single = len(levels) == 5 and not hasattr(levels[0][0], "__len__")
    res = []
    for lv in ([levels] if single else levels):
        if len(lv) != 5 or any(len(pair) != 2 for pair in lv):
            raise ValueError("msssim_from_levels: five (ssim, cs) pairs per image, got %r" % (lv,))
        terms = [float(lv[l][1]) for l in range(4)] + [float(lv[4][0])]
        res.append(float("nan") if any(not t >= 0 for t in terms) else math.prod(t ** w for t, w in zip(terms, MSSSIM_WEIGHTS)))
    return res[0] if single else res


def psnr_ssim_msssim(out, gt, value_range=(-1.0, 1.0)):
    """[(psnr, ssim, msssim), ...] per image, Python floats; psnr and ssim are exactly psnr_ssim's.  Inputs as for psnr_ssim, min(H, W) >= 176.  One
    device call (six launches) and one copy of 88 B bytes back."""
    import torch
    from . import ops
    _need_cuda("psnr_ssim_msssim", out, gt)
    buf = torch.empty(out.shape[0] if out.dim() == 4 else 1, 11, dtype=torch.float64, device=out.device)
    sse, levels = ops.image_msssim(out.contiguous(), gt.contiguous(), value_range=value_range, out=buf)
    n = out.numel() // sse.numel()
    host = buf.cpu().tolist()
    return [(psnr_from_sse(r[0], n), float(r[1]), msssim_from_levels([r[1 + 2 * l:3 + 2 * l] for l in range(5)])) for r in host]


def srgb_linear_table():
    """the 256 float32 values lin[v] of include/cfen_colordiff.h: with c = v / 255, c / 12.92 if c <= 0.04045, otherwise ((c + 0.055) / 1.055)^2.4,
    evaluated in float64 and rounded once; a numpy array (ops.image_ciede2000 uploads it once per device)"""
    import numpy as np
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)


def ciede2000(out, gt):
    """[mean dE00, ...] per image, Python floats.  out, gt: (B,H,W,3) / (H,W,3) uint8 CUDA tensors of equal shape, read as sRGB; out is colour 1.
    One device call (two launches) and one copy of 8 B bytes back."""
    import torch
    from . import ops
    _need_cuda("ciede2000", out, gt)
    return [float(v) for v in ops.image_ciede2000(out.contiguous(), gt.contiguous()).cpu().tolist()]


def parse_columns(text):
    """--eval_metrics: 'psnr,ssim' or 'psnr,ssim,msssim' -> the tuple of columns; psnr and ssim are always written, in the csv's fixed order"""
    names = [t.strip() for t in str(text).split(",") if t.strip()]
    for n in names:
        if n not in COLUMNS:
            raise ValueError("--eval_metrics: unknown metric '%s' (known: %s)%s" % (
                n, ", ".join(COLUMNS), "; CIEDE2000 has a flag of its own, --eval_ciede2000" if n == CIEDE_COLUMN else ""))
    if len(set(names)) != len(names) or "psnr" not in names or "ssim" not in names:
        raise ValueError("--eval_metrics: psnr and ssim are always written, each name once: psnr,ssim or psnr,ssim,msssim (got '%s')" % text)
    return tuple(c for c in COLUMNS if c in names)


def _fmt(v):
    return "inf" if math.isinf(v) else "nan" if math.isnan(v) else "%.6f" % v


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


# ---- the same three with the column list (--eval_metrics): rows are (image, value per column ...) ---------------------------------------------------
def csv_header(columns):
    return ",".join(("image",) + tuple(columns))


def format_csv_columns(rows, columns):
    """the text of metrics.csv for the given columns: %.6f, an infinite PSNR as `inf`, an undefined MS-SSIM as `nan`; for ('psnr', 'ssim') it is
    format_csv's text"""
    for r in rows:
        if len(r) != 1 + len(columns):
            raise ValueError("format_csv_columns: a row of %d values for the columns %s" % (len(r) - 1, ",".join(columns)))
    return "".join([csv_header(columns) + "\n"] + [",".join([str(r[0])] + [_fmt(v) for v in r[1:]]) + "\n" for r in rows])


def summarize_columns(rows, columns):
    """summarize() of the psnr and ssim columns, plus with 'msssim': 'msssim_mean' (over the rows that are not NaN, nan when there is none) and
    'msssim_nan' (how many are NaN), and with 'ciede2000': 'ciede2000_mean' (nan without rows)"""
    ip, iss = 1 + list(columns).index("psnr"), 1 + list(columns).index("ssim")
    s = summarize([(r[0], r[ip], r[iss]) for r in rows])
    if "msssim" in columns:
        im = 1 + list(columns).index("msssim")
        good = [r[im] for r in rows if not math.isnan(r[im])]
        s["msssim_mean"] = sum(good) / len(good) if good else float("nan")
        s["msssim_nan"] = len(rows) - len(good)
    if CIEDE_COLUMN in columns:
        ic = 1 + list(columns).index(CIEDE_COLUMN)
        s["ciede2000_mean"] = sum(r[ic] for r in rows) / len(rows) if rows else float("nan")
    return s


def summary_line_columns(rows, columns):
    ip, iss = 1 + list(columns).index("psnr"), 1 + list(columns).index("ssim")
    line = summary_line([(r[0], r[ip], r[iss]) for r in rows])
    if "msssim" in columns:
        s = summarize_columns(rows, columns)
        line += ", mean MS-SSIM %.6f over %d (%d nan)" % (s["msssim_mean"], s["images"] - s["msssim_nan"], s["msssim_nan"])
    if CIEDE_COLUMN in columns:
        line += ", mean CIEDE2000 %.4f" % summarize_columns(rows, columns)["ciede2000_mean"]
    return line


# ---- --eval_noref: statistics of the hazy input and the dehazed output, no ground truth (include/cfen_noref.h has the long form) ----------------
# Per image of the pair, from the luma Y = (77 R + 150 G + 29 B + 128) >> 8:
#   dark          mean of the dark channel (He, Sun and Tang 2009: min of min(R, G, B) over a (2 r + 1)^2 window clipped to the image) / 255
#   entropy       -sum p log2 p over the non-empty bins of the 256-bin histogram of Y, in bits
#   avg_gradient  mean over the (H - 1)(W - 1) positions of sqrt((dx^2 + dy^2) / 2), forward differences of Y on the 0..255 scale; nan without one
#   contrast      population standard deviation of Y / 255
# and for the pair: saturated, the share of pixels with Y_out in {0, 255} whose Y_hazy is not (sigma of Hautiere et al. 2008).
NOREF_COLUMNS = ("dark_in", "dark_out", "entropy_in", "entropy_out", "avg_gradient_in", "avg_gradient_out", "contrast_in", "contrast_out", "saturated")
NOREF_CSV_HEADER = "image," + ",".join(NOREF_COLUMNS)
NOREF_MAX_RADIUS = 16


def _noref_side(cnt, grad_sum, H, W):
    """(dark, entropy, avg_gradient, contrast) of one side from its 259 integers and its gradient sum"""
    n = H * W
    hist = [int(c) for c in cnt[:256]]
    if sum(hist) != n:
        raise ValueError("noref_from_stats: the histogram holds %d pixels, the image %d x %d" % (sum(hist), H, W))
    dark = int(cnt[256]) / (255.0 * n)
    s = 0.0
    for c in hist:
        if c:
            s += (c / n) * math.log2(c / n)
    s1 = sum(v * c for v, c in enumerate(hist))
    s2 = sum(v * v * c for v, c in enumerate(hist))
    contrast = math.sqrt((n * s2 - s1 * s1) / float(n * n)) / 255.0          # exact integers up to the one division
    positions = (H - 1) * (W - 1)
    return dark, 0.0 - s, (float(grad_sum) / positions if positions > 0 else float("nan")), contrast


def noref_from_stats(counts, grad, H, W):
    """the device's raw statistics -> [(dark_in, dark_out, entropy_in, entropy_out, avg_gradient_in, avg_gradient_out, contrast_in, contrast_out,
    saturated), ...] per image, Python floats in the order of NOREF_COLUMNS.  counts: (B,2,259) integers, grad: (B,2) floats (tensors, arrays
    or nested lists: ops.image_noref's results after .cpu()); float64 on the host, the way msssim_from_levels finishes MS-SSIM"""
    counts = counts.tolist() if hasattr(counts, "tolist") else counts
    grad = grad.tolist() if hasattr(grad, "tolist") else grad
    rows = []
    for c, g in zip(counts, grad):
        a, b = _noref_side(c[0], g[0], H, W), _noref_side(c[1], g[1], H, W)
        rows.append((a[0], b[0], a[1], b[1], a[2], b[2], a[3], b[3], int(c[1][257]) / float(H * W)))
    return rows


def noref(hazy, out, radius=7):
    """[NOREF_COLUMNS row, ...] per image pair.  hazy, out: (B,H,W,3) / (H,W,3) uint8 CUDA tensors of equal shape.  One device call (two
    launches) and one copy of B * 4160 bytes back."""
    import torch
    from . import ops
    _need_cuda("noref", hazy, out)
    counts, grad = ops.image_noref(hazy.contiguous(), out.contiguous(), radius)
    B = counts.shape[0]
    H, W = (hazy.shape[0], hazy.shape[1]) if hazy.dim() == 3 else (hazy.shape[1], hazy.shape[2])
    # one copy back: the doubles travel as their bit patterns beside the integers
    host = torch.cat([counts.view(B, -1), grad.view(torch.int64)], dim=1).cpu()
    return noref_from_stats(host[:, :518].view(B, 2, 259), host[:, 518:].contiguous().view(torch.float64), int(H), int(W))


def bytes_from_normalized(x):
    """the loader's normalised floats (B,3,H,W), (v / 255 - 0.5) / 0.5, back to the decoded bytes (B,H,W,3) uint8, by ROUNDING: the float chain
    lands within 1e-4 of v, and truncating (util.tensor2im) can come back one level low"""
    import torch
    return ((x.float() * 0.5 + 0.5) * 255.0).round().clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def format_noref_csv(rows):
    """[(image, *NOREF_COLUMNS values), ...] -> the text of noref.csv: header, then %.6f values, one row per image"""
    lines = [NOREF_CSV_HEADER]
    for r in rows:
        if len(r) != 1 + len(NOREF_COLUMNS):
            raise ValueError("format_noref_csv: a row has %d values for %d columns" % (len(r) - 1, len(NOREF_COLUMNS)))
        lines.append(",".join([str(r[0])] + ["%.6f" % v for v in r[1:]]))
    return "\n".join(lines) + "\n"


def summarize_noref(rows):
    """{column + '_mean': mean over the rows that are not nan (nan when there is none)} and 'images'"""
    s = {"images": len(rows)}
    for i, name in enumerate(NOREF_COLUMNS):
        good = [r[1 + i] for r in rows if not math.isnan(r[1 + i])]
        s[name + "_mean"] = sum(good) / len(good) if good else float("nan")
    return s


def noref_summary_line(rows):
    """the one line test.py --eval_noref prints (the contrast column is in the csv only)"""
    s = summarize_noref(rows)
    return ("noref: %d images, mean dark channel %.6f -> %.6f, mean entropy %.4f -> %.4f, mean avg gradient %.4f -> %.4f, mean saturated %.6f"
            % (s["images"], s["dark_in_mean"], s["dark_out_mean"], s["entropy_in_mean"], s["entropy_out_mean"],
               s["avg_gradient_in_mean"], s["avg_gradient_out_mean"], s["saturated_mean"]))
