"""The definition of include/cfen_flicker.h in numpy: what csrc/k_flicker.hip and flicker.Scorer compute (the integer sums of a frame pair along
block vectors, the scores formed from them, the Scorer composed with tests/motion_ref.py's search and tests/resample_ref.py's box filter), and
the cases that tests/test_flicker_host.py and tests/test_hip_flicker.py share.

Everything up to the final divisions is integer: there is exactly one right answer and no tolerance."""
import functools
import math

import numpy as np

import motion_ref
import resample_ref
import temporal_ref

CUT_SHARE = 0.5
FIELDS = ("motion", "covered", "matched", "cut", "hazy", "net", "out", "ewarp_net", "ewarp_out", "pixels", "n_matched", "sad_hazy", "sad_net", "sad_out",
          "sq_net", "sq_out")


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------------------
def sums_one(I, Ip, F, Fp, vec, block, tol):
    """I, Ip, F, Fp (h, w, 3) uint8, vec (bh, bw, 2) int16 or None -> the eight int64 of one frame pair.  q = p + v_b is NOT clamped: a pixel whose
    q lies outside the frame is not covered"""
    h, w = I.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    v = np.zeros((h, w, 2), np.int64) if vec is None else np.asarray(vec).astype(np.int64)[y // block, x // block]
    qy, qx = y + v[..., 0], x + v[..., 1]
    cov = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    sy, sx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)                                   # (only read where covered)
    di = np.abs(I.astype(np.int64) - Ip[sy, sx]).sum(axis=2)
    d = F.astype(np.int64) - Fp[sy, sx]
    df, ef = np.abs(d).sum(axis=2), (d * d).sum(axis=2)
    m = cov & (di <= 3 * tol)
    return np.array([cov.sum(), m.sum(), di[m].sum(), df[m].sum(), ef[m].sum(), df[cov].sum(), di[cov].sum(), 0], np.int64)


def sums(guide, prev_guide, tgt, prev_tgt, vec, block, tol):
    """guide, tgt (B, h, w, 3), prev_guide, prev_tgt (h, w, 3), vec (B, bh, bw, 2) or None -> (B, 8) int64; the predecessor of frame k is frame
    k - 1 of the call, of frame 0 it is prev_guide / prev_tgt"""
    return np.stack([sums_one(guide[k], guide[k - 1] if k else prev_guide, tgt[k], tgt[k - 1] if k else prev_tgt, None if vec is None else vec[k],
                              block, tol) for k in range(len(guide))])


def sums_plain(I, Ip, F, Fp, vec, block, tol):
    """the same by a loop over pixels"""
    h, w = I.shape[:2]
    s = [0] * 8
    for y in range(h):
        for x in range(w):
            dy, dx = (0, 0) if vec is None else (int(c) for c in vec[y // block, x // block])
            qy, qx = y + dy, x + dx
            if not (0 <= qy < h and 0 <= qx < w):
                continue
            di = sum(abs(int(I[y, x, c]) - int(Ip[qy, qx, c])) for c in range(3))
            df = sum(abs(int(F[y, x, c]) - int(Fp[qy, qx, c])) for c in range(3))
            ef = sum((int(F[y, x, c]) - int(Fp[qy, qx, c])) ** 2 for c in range(3))
            s[0] += 1
            s[5] += df
            s[6] += di
            if di <= 3 * tol:
                s[1] += 1
                s[2] += di
                s[3] += df
                s[4] += ef
    return np.array(s, np.int64)


# ---- the scores -------------------------------------------------------------------------------------------------------------------------------------
def scores(s, h, w):
    """(flicker, hazy, ewarp, covered, matched) of one frame pair's sums, float64; nan where nothing is matched"""
    s = [int(v) for v in s]
    n = s[1]
    if n == 0:
        return math.nan, math.nan, math.nan, s[0] / (h * w), 0.0
    return s[3] / (3 * n), s[2] / (3 * n), s[4] / (3 * n * 255 ** 2), s[0] / (h * w), n / (h * w)


def row(s_net, s_out, vec, block, h, w):
    """one row of flicker.csv as a dict over FIELDS"""
    a, b = scores(s_net, h, w), scores(s_out, h, w)
    bh, bw = -(-h // block), -(-w // block)
    l1 = 0 if vec is None else int(np.abs(np.asarray(vec).astype(np.int64)).sum())
    return dict(zip(FIELDS, (l1 / (bh * bw), a[3], a[4], int(a[4] < CUT_SHARE), a[1], a[0], b[0], a[2], b[2], h * w, int(s_net[1]), int(s_net[2]),
                             int(s_net[3]), int(s_out[3]), int(s_net[4]), int(s_out[4]))))


def pooled(rows, key="sad_net", scale=1.0):
    """sum_rows sums / (3 sum_rows n_match) over the rows that are no cut, as motion_ref.flicker_along_motion pools"""
    good = [r for r in rows if not r["cut"]]
    n = sum(r["n_matched"] for r in good)
    return sum(r[key] for r in good) / (3 * n * scale) if n else math.nan


class Scorer:
    """flicker.Scorer on the host, any batching: step(G, N, O=None) -> rows; field(I, I_prev) -> vec, when given, replaces the search"""

    def __init__(self, range=8, block=16, bias=4, tol=8, down="auto", field=None):
        self.range, self.block, self.bias, self.tol, self.down, self.field = range, block, bias, tol, down, field
        self.prev = None

    def step(self, G, N, O=None):
        O = N if O is None else O
        H, W = G.shape[1:3]
        S, h, w = temporal_ref.working_size(H, W, self.down)
        rows = []
        for k in range(len(G)):
            cur = tuple(f[k] if S == 1 else resample_ref.pil_resize(f[k], (h, w), "box") for f in (G, N, O))
            if self.prev is not None:
                vec = None
                if self.field is not None:
                    vec = self.field(cur[0], self.prev[0])
                elif self.range:
                    vec = motion_ref.search_one(cur[0], self.prev[0], self.block, self.range, self.bias)[0]
                s_net = sums_one(cur[0], self.prev[0], cur[1], self.prev[1], vec, self.block, self.tol)
                s_out = sums_one(cur[0], self.prev[0], cur[2], self.prev[2], vec, self.block, self.tol)
                rows.append(row(s_net, s_out, vec, self.block, h, w))
            self.prev = cur
        return rows


# ---- the cases of tests/test_hip_flicker.py ---------------------------------------------------------------------------------------------------------
SIZES = motion_ref.SIZES
BLOCKS = motion_ref.BLOCKS
TOLS = (0, 8, 255)
KINDS = ("random", "shift", "flat")
FIELD_KINDS = ("null", "searched", "random", "extreme")


def field(kind, guide, prev_guide, block, seed):
    """vec (B, bh, bw, 2) int16 or None for the B frames guide behind prev_guide"""
    B, h, w = guide.shape[:3]
    bh, bw, _ = motion_ref.grid(h, w, block)
    rs = np.random.RandomState(seed)
    if kind == "null":
        return None
    if kind == "searched":
        return motion_ref.search(guide, prev_guide, block, 3, 4)[0]
    if kind == "random":
        return rs.randint(-16, 17, (B, bh, bw, 2)).astype(np.int16)
    return rs.choice(np.array([-32768, -32767, 32767], np.int16), size=(B, bh, bw, 2))          # coverage 0: every score nan


def _seed(*key):
    return sum((i + 1) * int(v) for i, v in enumerate(key)) * 41 % 100000


@functools.lru_cache(maxsize=None)
def sums_case(kind, fkind, h, w, block, B):
    """guide, prev_guide, tgt, prev_tgt, vec and {tol: sums (B, 8)} for every tol of TOLS; computed once, read-only.  The target is the guide
    plus a jitter of a few levels per frame and channel, so that dF differs from dI"""
    seed = _seed(KINDS.index(kind), FIELD_KINDS.index(fkind), h, w, block, B)
    f = motion_ref.frames(kind, h, w, B, seed)
    rs = np.random.RandomState(seed + 1)
    t = np.clip(f.astype(np.int64) + rs.randint(-9, 10, (B + 1, 1, 1, 3)) + rs.randint(-2, 3, f.shape), 0, 255).astype(np.uint8)
    vec = field(fkind, f[1:], f[0], block, seed + 2)
    want = {tol: sums(f[1:], f[0], t[1:], t[0], vec, block, tol) for tol in TOLS}
    out = (f[1:], f[0], t[1:], t[0], vec, want)
    for a in out[:5] + tuple(want.values()):
        if a is not None:
            a.setflags(write=False)
    return out
