"""Flicker along the motion of a dehazed stream (include/cfen_flicker.h states the definition).

A Scorer looks every block of the working-resolution hazy frame up in the previous one (ops.motion_search_u8, the search temporal.Stabiliser
uses, with vectors of its own) and sums, over the pixels whose hazy bytes did not change along those vectors, how much the network's frames and
the frames that leave did (ops.flicker_u8).  The sums are integers; the scores are formed from them on the host in float64.  Two runs of the
same clip with different --temporal settings are scored over the same pixels, so their figures are comparable.  Everything runs on the current
stream; step() waits for its own results and for nothing else."""
import math

from . import temporal

# block and bias are temporal.MC_DEFAULTS, range 8 is the README's --temporal_mc 8, tol 8 the motion threshold of DESIGN section 18
DEFAULTS = dict(range=8, block=16, bias=4, tol=8, down="auto")
CUT_SHARE = 0.5          # a frame pair of which less than this share is matched is a cut: marked, and left out of every pooled mean

CSV_HEADER = "frame,motion,covered,matched,cut,hazy,net,out,ewarp_net,ewarp_out,pixels,n_matched,sad_hazy,sad_net,sad_out,sq_net,sq_out"
ROW_FIELDS = tuple(CSV_HEADER.split(",")[1:])
_FLOATS = ("motion", "covered", "matched", "hazy", "net", "out", "ewarp_net", "ewarp_out")


def check_params(range, block, bias, tol, down, what="Scorer"):
    """(range, block, bias, tol, down) as ints, down an int or 'auto'; ValueError naming the argument out of range"""
    out = []
    for name, v, ok, say in (("range", range, lambda i: 0 <= i <= 16, "an integer in 0 .. 16 (0 = the zero field)"),
                             ("block", block, lambda i: i in (8, 16, 32), "8, 16 or 32"),
                             ("bias", bias, lambda i: 0 <= i <= 255, "an integer in 0 .. 255"),
                             ("tol", tol, lambda i: 0 <= i <= 255, "an integer in 0 .. 255")):
        try:
            i = int(v)
        except (TypeError, ValueError, OverflowError):
            i = None
        if i is None or i != v or not ok(i):
            raise ValueError("%s: %s must be %s, got %r" % (what, name, say, v))
        out.append(i)
    if down != "auto":
        try:
            d = int(down)
        except (TypeError, ValueError, OverflowError):
            d = None
        if d is None or d != down or d < 1:
            raise ValueError("%s: down must be 'auto' or an integer >= 1, got %r" % (what, down))
        down = d
    return tuple(out) + (down,)


def scores_from_sums(sums, h, w):
    """the eight integers of one frame pair (include/cfen_flicker.h) -> {flicker, hazy, ewarp, covered, matched}, Python floats; the first three
    are nan where nothing is matched"""
    s = [int(v) for v in sums]
    n = s[1]
    nan = float("nan")
    return {"flicker": s[3] / (3.0 * n) if n else nan, "hazy": s[2] / (3.0 * n) if n else nan, "ewarp": s[4] / (3.0 * n * 255.0 * 255.0) if n else nan,
            "covered": s[0] / float(h * w), "matched": s[1] / float(h * w)}


def row_from_sums(sums_net, sums_out, motion_l1, nblocks, h, w):
    """one row of flicker.csv (a dict over ROW_FIELDS) from the sums of the network's frames, of the frames that leave, the sum over blocks of
    |dy| + |dx| and the number of blocks"""
    a, b = scores_from_sums(sums_net, h, w), scores_from_sums(sums_out, h, w)
    return {"motion": int(motion_l1) / float(nblocks), "covered": a["covered"], "matched": a["matched"], "cut": int(a["matched"] < CUT_SHARE),
            "hazy": a["hazy"], "net": a["flicker"], "out": b["flicker"], "ewarp_net": a["ewarp"], "ewarp_out": b["ewarp"], "pixels": h * w,
            "n_matched": int(sums_net[1]), "sad_hazy": int(sums_net[2]), "sad_net": int(sums_net[3]), "sad_out": int(sums_out[3]),
            "sq_net": int(sums_net[4]), "sq_out": int(sums_out[4])}


def pool(rows):
    """the pooled figures of a clip: sums over the rows that are no cut, divided once.  {pairs, cuts, matched, hazy, net, out, ewarp_net, ewarp_out}"""
    good = [r for r in rows if not r["cut"]]
    n = sum(r["n_matched"] for r in good)
    px = sum(r["pixels"] for r in good)
    nan = float("nan")

    def mean(key, scale=1.0):
        return sum(r[key] for r in good) / (3.0 * n * scale) if n else nan
    return {"pairs": len(rows), "cuts": len(rows) - len(good), "matched": n / float(px) if px else nan, "hazy": mean("sad_hazy"), "net": mean("sad_net"),
            "out": mean("sad_out"), "ewarp_net": mean("sq_net", 255.0 * 255.0), "ewarp_out": mean("sq_out", 255.0 * 255.0)}


def _f(v):
    return "nan" if math.isnan(v) else "%.6f" % v


def format_csv(named_rows):
    """[(frame name, row), ...] -> the text of flicker.csv: header, then one line per frame pair; floats as %.6f, nan as nan, the rest integers"""
    lines = [CSV_HEADER]
    for name, r in named_rows:
        lines.append(",".join([str(name)] + [_f(r[k]) if k in _FLOATS else "%d" % r[k] for k in ROW_FIELDS]))
    return "\n".join(lines) + "\n"


def summary_line(rows):
    """the one line dehaze_video.py --eval_flicker prints"""
    p = pool(rows)
    ratio = p["out"] / p["net"] if p["net"] and not math.isnan(p["net"]) else float("nan")
    return ("flicker: %d frame pairs (%d cuts left out), matched %s %%, hazy %s, network %s -> out %s levels along the motion (B/A = %s), E_warp %s -> %s"
            % (p["pairs"], p["cuts"], "nan" if math.isnan(p["matched"]) else "%.1f" % (100.0 * p["matched"]),
               *("nan" if math.isnan(v) else "%.3f" % v for v in (p["hazy"], p["net"], p["out"], ratio)), _f(p["ewarp_net"]), _f(p["ewarp_out"])))


class Scorer:
    """step(hazy_u8, net_u8, out_u8=None) for consecutive batches of consecutive frames, (n,H,W,3) uint8 CUDA tensors: one row (a dict over
    ROW_FIELDS) per frame that has a predecessor -- the first frame after construction or reset() yields none.  The object keeps copies of the
    last working-resolution hazy, network and output frame; the rows do not depend on how the frames are grouped into batches.  range = 0 scores
    with the zero field and launches no search; otherwise one ops.motion_search_u8 per call, then one ops.flicker_u8 per target (one in all
    when out_u8 is None or net_u8 itself).  The vectors are the Scorer's own, never a Stabiliser's."""

    def __init__(self, range=DEFAULTS["range"], block=DEFAULTS["block"], bias=DEFAULTS["bias"], tol=DEFAULTS["tol"], down=DEFAULTS["down"]):
        self.range, self.block, self.bias, self.tol, self.down = check_params(range, block, bias, tol, down)
        self.reset()

    def reset(self):
        """the next frame is the first of a stream (frames of another size may follow)"""
        self._key = None
        self._prev = None          # (hazy, network, output) at the working resolution; the last two are one tensor while out_u8 is net_u8

    def working_size(self, H, W):
        """(S, h, w): the factor and the working resolution of H x W frames, temporal.working_size's rule"""
        return temporal.working_size(H, W, self.down)

    def step(self, hazy_u8, net_u8, out_u8=None):
        import torch
        from . import ops
        if out_u8 is net_u8:
            out_u8 = None
        given = (("hazy_u8", hazy_u8), ("net_u8", net_u8)) + ((("out_u8", out_u8),) if out_u8 is not None else ())
        for name, t in given:
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8 or min(t.shape) < 1 or not t.is_cuda or \
                    not t.is_contiguous():
                raise ValueError("Scorer.step needs %s as a contiguous (n,H,W,3) uint8 CUDA tensor, got %s"
                                 % (name, "%s %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
            if t.shape != hazy_u8.shape or t.device != hazy_u8.device:
                raise ValueError("Scorer.step: hazy_u8 %s and %s %s differ in shape or device" % (tuple(hazy_u8.shape), name, tuple(t.shape)))
        n, H, W, _ = hazy_u8.shape
        dev = hazy_u8.device
        key = (H, W, dev)
        if self._key is not None and key != self._key:
            raise ValueError("Scorer.step: frames of %d x %d on %s after frames of %d x %d on %s: reset() starts a new stream"
                             % (H, W, dev, self._key[0], self._key[1], self._key[2]))
        self._key = key
        S, h, w = self.working_size(H, W)
        small = (lambda t: t) if S == 1 else (lambda t: ops.resample_u8(t, (h, w), filter="box"))
        I, N = small(hazy_u8), small(net_u8)
        O = N if out_u8 is None else small(out_u8)
        first = 1 if self._prev is None else 0          # the first frame of a stream has no predecessor
        rows = []
        if first < n:
            pI, pN, pO = (I[0], N[0], O[0]) if first else self._prev
            vec = ops.motion_search_u8(I[first:], pI, self.block, self.range, self.bias)[0] if self.range else None
            sums = [ops.flicker_u8(I[first:], pI, N[first:], pN, vec, self.block, self.tol)]
            sums.append(sums[0] if O is N and pO is pN else ops.flicker_u8(I[first:], pI, O[first:], pO, vec, self.block, self.tol))
            m = n - first
            l1 = vec.to(torch.int64).abs().sum(dim=(1, 2, 3)) if vec is not None else torch.zeros(m, dtype=torch.int64, device=dev)
            host = torch.cat([sums[0], sums[1], l1[:, None]], dim=1).cpu().tolist()          # one copy back, which waits for the launches above
            nblocks = -(-h // self.block) * -(-w // self.block)
            rows = [row_from_sums(r[:8], r[8:16], r[16], nblocks, h, w) for r in host]
        last = (I[n - 1].clone(), N[n - 1].clone())
        self._prev = last + (last[1] if O is N else O[n - 1].clone(),)
        return rows
