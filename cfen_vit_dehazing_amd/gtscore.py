"""Scores of a dehazed stream against a ground-truth stream (include/cfen_planes.h states the definition).

The video world's convention: per plane on the samples as they are stored -- PSNR-Y / Cb / Cr, an "average" PSNR from the summed squared
errors of all planes (what ffmpeg's psnr filter calls average), SSIM per plane -- and beside them a temporal error, how far the output's
change from one frame to the next is from the ground truth's own.  A Scorer hands each batch of payloads to ops.plane_metrics and keeps the
last frame pair on the device for the next batch.  The device returns integers and one double per plane; every figure below is formed from
them on the host in float64, so a row does not depend on how the frames were grouped into batches.  Everything runs on the current stream;
step() waits for its own results and for nothing else."""
import math

CSV_HEADER = "frame,psnr_y,psnr_cb,psnr_cr,psnr_avg,ssim_y,ssim_cb,ssim_cr,dt_y,sse_y,sse_cb,sse_cr,dtsum_y,n_y,n_c"
PLANES = ("y", "cb", "cr")


def psnr(sse, count, depth):
    """10 log10(top^2 count / sse) with top = 2^depth - 1; inf for sse = 0, nan for a plane that is not there (count = 0)"""
    if count == 0:
        return float("nan")
    if sse == 0:
        return float("inf")
    top = float((1 << depth) - 1)
    return 10.0 * math.log10(top * top * count / sse)


def row_from_words(sse, dt, ssim, count, depth, has_prev):
    """one frame's row (a dict) from the three planes' words of cfen_plane_metrics; has_prev: the frame had a predecessor"""
    sse, dt, count = [int(v) for v in sse], [int(v) for v in dt], [int(v) for v in count]
    return {"depth": depth, "sse": sse, "count": count, "ssim": [float(v) for v in ssim], "dtsum_y": dt[0] if has_prev else None,
            "psnr": [psnr(s, n, depth) for s, n in zip(sse, count)], "psnr_avg": psnr(sum(sse), sum(count), depth),
            "dt_y": dt[0] / float(count[0]) if has_prev else None}


def pool(rows):
    """the pooled figures of a clip, from the summed integers: {frames, psnr_y, psnr_avg, ssim_y, dt_y}.  Pooling the PSNR from sums keeps an
    identical frame's inf out of a mean; dt_y is sum DT_y / sum count_y over the frames that have a predecessor (nan if none has)"""
    nan = float("nan")
    if not rows:
        return {"frames": 0, "psnr_y": nan, "psnr_avg": nan, "ssim_y": nan, "dt_y": nan}
    depth = rows[0]["depth"]
    timed = [r for r in rows if r["dtsum_y"] is not None]
    n_t = sum(r["count"][0] for r in timed)
    return {"frames": len(rows), "psnr_y": psnr(sum(r["sse"][0] for r in rows), sum(r["count"][0] for r in rows), depth),
            "psnr_avg": psnr(sum(sum(r["sse"]) for r in rows), sum(sum(r["count"]) for r in rows), depth),
            "ssim_y": sum(r["ssim"][0] for r in rows) / len(rows), "dt_y": sum(r["dtsum_y"] for r in timed) / float(n_t) if n_t else nan}


def _f(v, fmt="%.6f"):
    return "nan" if math.isnan(v) else ("inf" if math.isinf(v) else fmt % v)


def format_csv(named_rows):
    """[(frame name, row), ...] -> the text of gt.csv: header, then one line per frame.  PSNR in dB as %.6f (inf for equal planes), SSIM as
    %.9f, nan for a plane that is absent or too small for a window, dt_y in levels as %.6f and empty for a frame without a predecessor; then
    the integers the figures were formed from, for pooling over other sets of frames"""
    lines = [CSV_HEADER]
    for name, r in named_rows:
        lines.append(",".join([str(name)] + [_f(v) for v in r["psnr"]] + [_f(r["psnr_avg"])] + [_f(v, "%.9f") for v in r["ssim"]] +
                              ["" if r["dt_y"] is None else _f(r["dt_y"])] + ["%d" % v for v in r["sse"]] +
                              ["%d" % (r["dtsum_y"] or 0), "%d" % r["count"][0], "%d" % r["count"][1]]))
    return "\n".join(lines) + "\n"


def summary_line(rows):
    """the one line dehaze_video.py --eval_gt prints"""
    p = pool(rows)
    return ("gt: %d frames, PSNR-Y %s, mean SSIM-Y %s, PSNR avg %s, mean temporal error %s levels"
            % (p["frames"], _f(p["psnr_y"], "%.3f"), _f(p["ssim_y"]), _f(p["psnr_avg"], "%.3f"), _f(p["dt_y"], "%.4f")))


class Scorer:
    """step(out_frames, gt_frames) for consecutive batches of consecutive frames, (n, frame_bytes) uint8 CUDA tensors holding y4m payloads of
    H x W frames of `chroma` at `depth` bits per sample: one row per frame.  The object keeps copies of the last frame pair; the first frame
    after construction or reset() has no predecessor.  One ops.plane_metrics call per step."""

    def __init__(self, H, W, chroma, depth=8):
        from . import yuv
        yuv.chroma_code(chroma)
        self.H, self.W, self.chroma, self.depth = int(H), int(W), chroma, yuv.check_depth(depth)
        self.frame_bytes = yuv.frame_bytes(self.H, self.W, chroma, self.depth)
        self.reset()

    def reset(self):
        """the next frame is the first of a stream"""
        self._prev = None

    def step(self, out_frames, gt_frames):
        import torch
        from . import ops
        sse, dt, ssim, count = ops.plane_metrics(out_frames, gt_frames, self.H, self.W, self.chroma, self.depth, prev=self._prev)
        n = out_frames.shape[0]
        host = torch.cat([sse, dt, count], dim=1).cpu().tolist()          # the copies back wait for the launches above
        ssim = ssim.cpu().tolist()
        rows = [row_from_words(host[k][0:3], host[k][3:6], ssim[k], host[k][6:9], self.depth, has_prev=(k > 0 or self._prev is not None))
                for k in range(n)]
        self._prev = (out_frames[n - 1].clone(), gt_frames[n - 1].clone())
        return rows
