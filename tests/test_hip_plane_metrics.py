"""Per-plane scores against a ground-truth stream on the device (cfen_plane_metrics; ops.plane_metrics, gtscore.Scorer).  The integers are held
to the restatement tests/planes_ref.py bit for bit; the mean SSIM to its float64 value with the bar of tests/test_hip_metrics.py, 2 D, where D
is the distance of an fp32 evaluation of the same definition from float64: at depth 8 the reference's own (max_ref32_f64 of
tests/golden/metrics_pairs.npz), at the deeper depths the one of an fp32 numpy evaluation over this file's own pairs, computed here on the CPU.

CFEN_WRITE_PARITY=1 writes the distances and the bars to profiles/plane_metrics_parity.json.

The kernel forms its fp32 maps from centred samples (include/cfen_planes.h), which is what keeps a plane of ONE window -- 11 x 11 Cmono, the
11 x 11 chroma of 21 x 22 C420jpeg, where no averaging hides the map's rounding -- inside the depth-8 bar."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, gtscore, ops
import guarded
import planes_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEVERAL_TILES = (130, 259, "420jpeg")          # luma 5 x 4 tiles, chroma 65 x 130: 3 x 2 tiles, partial tiles on both edges
# the smallest shapes that can go wrong: one window; chroma of 11 x 12 and 11 x 11; chroma 10 high (no window); 4:2:2; 4:4:4 with odd sizes; tiles
SHAPES = ((11, 11, "mono"), (22, 23, "420jpeg"), (21, 22, "420jpeg"), (20, 22, "420mpeg2"), (12, 23, "422"), (17, 33, "444"), SEVERAL_TILES)
DEPTHS = (8, 10, 16)
CASES = [(H, W, c, d) for H, W, c in SHAPES for d in DEPTHS] + [(17, 33, "444", d) for d in (9, 12, 14)]
B = 3


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared reference arrays are read-only


@functools.lru_cache(maxsize=None)
def want(H, W, chroma, depth, kind="noisy", dtype="f64"):
    """the restatement's words of the B frames of a pair, computed once and shared"""
    a, b = ref.pair(H, W, chroma, depth, B, 1000 * H + W + depth, kind)
    return ref.words(a, b, H, W, chroma, depth, dtype=np.float64 if dtype == "f64" else np.float32)


def frames(H, W, chroma, depth, kind="noisy"):
    return ref.pair(H, W, chroma, depth, B, 1000 * H + W + depth, kind)


@functools.lru_cache(maxsize=None)
def distance(deep):
    """D: depth 8 -> the golden file's; deeper -> max |fp32 numpy - float64| over every deep noisy pair of this file"""
    if not deep:
        return float(np.load(os.path.join(ROOT, "tests", "golden", "metrics_pairs.npz"))["max_ref32_f64"])
    d = 0.0
    for H, W, c, depth in CASES:
        if depth > 8:
            diff = np.abs(want(H, W, c, depth)[2] - want(H, W, c, depth, dtype="f32")[2])
            d = max(d, float(np.nanmax(diff)))
    assert d > 0.0
    return d


_WORST = {}


def _record(depth, case, d64):
    dist = distance(depth > 8)
    w = _WORST.setdefault("depth_%d" % depth, {"worst_abs_diff_from_f64": 0.0, "worst_case": None, "D": dist, "bar_f64": 2 * dist})
    if d64 >= w["worst_abs_diff_from_f64"]:
        w["worst_abs_diff_from_f64"], w["worst_case"] = d64, case
    if os.environ.get("CFEN_WRITE_PARITY") == "1":
        with open(os.path.join(ROOT, "profiles", "plane_metrics_parity.json"), "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "D_depth_8_golden_max_ref32_f64": distance(False),
                       "D_deep_fp32_numpy_over_this_files_pairs": distance(True), "depths": _WORST}, f, indent=1, sort_keys=True)
            f.write("\n")


def check(got, wanted, depth, case):
    """got: the four (n,3) tensors of ops.plane_metrics; wanted: the restatement's.  Integers bitwise, SSIM within 2 D, NaN where NaN"""
    sse, dt, ssim, count = (t.cpu().numpy() for t in got)
    assert sse.dtype == dt.dtype == count.dtype == np.int64 and ssim.dtype == np.float64 and sse.shape == ssim.shape == wanted[0].shape
    assert np.array_equal(sse, wanted[0]), (case, sse, wanted[0])
    assert np.array_equal(dt, wanted[1]), (case, dt, wanted[1])
    assert np.array_equal(count, wanted[3]), (case, count, wanted[3])
    assert np.array_equal(np.isnan(ssim), np.isnan(wanted[2])), (case, ssim, wanted[2])
    bar = 2 * distance(depth > 8)
    d64 = float(np.nanmax(np.abs(ssim - wanted[2]))) if not np.isnan(wanted[2]).all() else 0.0
    print("%s: max |ssim - f64| %.3e (bar %.3e)" % (case, d64, bar))
    _record(depth, str(case), d64)
    assert d64 <= bar, (case, d64, bar)


def run(a, b, H, W, chroma, depth, prev=None):
    return ops.plane_metrics(a, b, H, W, chroma, depth, prev=prev)


# ---- the words -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,chroma,depth", CASES)
def test_words(H, W, chroma, depth):
    """seeded noise: a batch of 3 (frames 1 and 2 have a predecessor), and frame 2 alone behind frame 1 through prev"""
    a, b = frames(H, W, chroma, depth)
    ta, tb = dev(a), dev(b)
    w = want(H, W, chroma, depth)
    assert (w[1][1:, 0] > 0).all() and not w[1][0].any()
    got = run(ta, tb, H, W, chroma, depth)
    check(got, w, depth, (H, W, chroma, depth))
    one = run(ta[2:], tb[2:], H, W, chroma, depth, prev=(ta[1], tb[1]))
    assert torch.equal(_bits(one), _bits(got)[2:])                # NaN bits included


@pytest.mark.parametrize("H,W,chroma,depth", [(22, 23, "420jpeg", 8), (17, 33, "444", 10), (130, 259, "420jpeg", 16), (20, 22, "420mpeg2", 12)])
def test_content_edges(H, W, chroma, depth):
    """a pair differing in one sample; equal frames; values above top"""
    a, b = frames(H, W, chroma, depth, "one_sample")
    w = want(H, W, chroma, depth, "one_sample")
    assert w[0][:2].sum() == 0 and w[0][2, 0] > 0 and not w[0][2, 1:].any() and w[1][2, 0] > 0 and not w[1][1].any()
    got = run(dev(a), dev(b), H, W, chroma, depth)
    check(got, w, depth, (H, W, chroma, depth, "one_sample"))
    ssim = got[2].cpu().numpy()
    assert (ssim[:2][~np.isnan(ssim[:2])] == 1.0).all() and ssim[2, 0] < 1.0
    a, b = frames(H, W, chroma, depth, "equal")
    got = run(dev(a), dev(b), H, W, chroma, depth)
    sse, dt, ssim, count = (t.cpu().numpy() for t in got)
    assert not sse.any() and not dt.any() and (ssim[~np.isnan(ssim)] == 1.0).all() and np.array_equal(count, want(H, W, chroma, depth)[3])
    assert all(gtscore.psnr(int(s), int(n), depth) == float("inf") for s, n in zip(sse[:, 0], count[:, 0]))
    same = dev(a)
    got = run(same, same, H, W, chroma, depth)                    # a stream against itself, through the same pointer
    assert not got[0].any() and not got[1].any()
    if 8 < depth < 16:
        a, b = frames(H, W, chroma, depth, "over_top")
        assert (a.view("<u2") > ref.top(depth)).any() and (b.view("<u2") > ref.top(depth)).any()
        check(run(dev(a), dev(b), H, W, chroma, depth), want(H, W, chroma, depth, "over_top"), depth, (H, W, chroma, depth, "over_top"))


@pytest.mark.parametrize("H,W,chroma", [(22, 23, "420jpeg"), SEVERAL_TILES])
def test_all_top_against_all_zero_at_16_bits(H, W, chroma):
    """SSE = top^2 N exactly: a tile's sum passes 2^32 and a thread's own does"""
    a, b = frames(H, W, chroma, 16, "extremes")
    got = run(dev(a), dev(b), H, W, chroma, 16)
    sse, dt, ssim, count = (t.cpu().numpy() for t in got)
    n = np.array([h * w for h, w in ref.plane_shapes(H, W, chroma)], dtype=np.int64)
    assert np.array_equal(count, np.tile(n, (B, 1))) and np.array_equal(sse, np.tile(65535 ** 2 * n, (B, 1))) and 65535 ** 2 * 34 * 74 > 1 << 32
    assert not dt.any()                                           # out - gt is top in every frame
    check(got, want(H, W, chroma, 16, "extremes"), 16, (H, W, chroma, 16, "extremes"))


# ---- batch, streams, strides, alignment --------------------------------------------------------------------------------------------------------------
def _bits(got):
    return torch.stack([got[0], got[1], got[2].contiguous().view(torch.int64), got[3]], dim=2).cpu()


@pytest.mark.parametrize("H,W,chroma,depth", [(130, 259, "420jpeg", 8), (130, 259, "420jpeg", 10), (21, 22, "420jpeg", 16), (11, 11, "mono", 8)])
def test_a_batch_is_its_frames_chained_through_prev_on_any_stream(H, W, chroma, depth):
    a, b = frames(H, W, chroma, depth)
    ta, tb = dev(a), dev(b)
    whole = _bits(run(ta, tb, H, W, chroma, depth))
    singles = [_bits(run(ta[k:k + 1], tb[k:k + 1], H, W, chroma, depth, prev=(ta[k - 1], tb[k - 1]) if k else None)) for k in range(B)]
    assert torch.equal(torch.cat(singles), whole)
    assert torch.equal(_bits(run(ta, tb, H, W, chroma, depth)), whole)                             # a repeated call
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = run(ta, tb, H, W, chroma, depth)
    side.synchronize()
    assert torch.equal(_bits(there), whole)
    # gtscore.Scorer over any grouping of the frames: the same rows
    rows = lambda sizes: [r for sc in [gtscore.Scorer(H, W, chroma, depth)] for lo, n in sizes for r in sc.step(ta[lo:lo + n], tb[lo:lo + n])]
    all3 = rows([(0, 3)])
    key = lambda rs: [(r["sse"], r["count"], r["dtsum_y"], [repr(v) for v in r["ssim"]], gtscore.format_csv([("f", r)])) for r in rs]
    for other in (rows([(0, 1), (1, 1), (2, 1)]), rows([(0, 2), (2, 1)])):
        assert len(other) == 3 and key(other) == key(all3)
    assert all3[0]["dt_y"] is None and all3[1]["dtsum_y"] == int(whole[1, 0, 1])
    sc = gtscore.Scorer(H, W, chroma, depth)
    sc.step(ta[:1], tb[:1])
    sc.reset()
    assert sc.step(ta[1:2], tb[1:2])[0]["dt_y"] is None


def _placed(rows, offset, gap):
    """the (B, nb) rows in a buffer of their own: first byte `offset` bytes behind a 16-byte boundary, rows nb + gap bytes apart"""
    n, nb = rows.shape
    buf = torch.zeros(16 + offset + n * (nb + gap), dtype=torch.uint8, device=DEV)
    start = (-buf.data_ptr()) % 16 + offset
    view = buf[start:start + n * (nb + gap)].view(n, nb + gap)[:, :nb]
    view.copy_(dev(rows))
    assert view.data_ptr() % 16 == offset and (n == 1 or view.stride(0) == nb + gap)
    return view


@pytest.mark.parametrize("H,W,chroma,depth", [(22, 23, "420jpeg", 8), (130, 259, "420jpeg", 8), (17, 33, "444", 10), (130, 259, "420jpeg", 16), (21, 22, "420jpeg", 12)])
def test_strides_and_byte_offsets(H, W, chroma, depth):
    """stride = frame_bytes + 6; frames at byte offset 1 (depth 8) and 2 (deep), each buffer alone and all together: the same bits"""
    a, b = frames(H, W, chroma, depth)
    ta, tb = dev(a), dev(b)
    base = _bits(run(ta[1:], tb[1:], H, W, chroma, depth, prev=(ta[0], tb[0])))
    k = 1 if depth == 8 else 2
    for oa, ob, opa, opb, gap in ((0, 0, 0, 0, 6), (k, 0, 0, 0, 0), (0, k, 0, 0, 0), (0, 0, k, 0, 0), (0, 0, 0, k, 0), (k, k, k, k, 6), (k, 3 * k, 2 * k, 5 * k, 6)):
        pa, pb = _placed(a[1:], oa, gap), _placed(b[1:], ob, gap)
        qa, qb = _placed(a[:1], opa, 0)[0], _placed(b[:1], opb, 0)[0]
        assert torch.equal(_bits(run(pa, pb, H, W, chroma, depth, prev=(qa, qb))), base), (oa, ob, opa, opb, gap)


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_plane_metrics():
    """every input between 0xff bands, out and scratch between random bands and prefilled with 0xff (NaN bits), zeros and random bytes: no band
    changes and the words are the same whatever the two held before"""
    lib = _lib.load()
    for (H, W, chroma, depth), with_prev in (((130, 259, "420jpeg", 8), True), ((21, 22, "420jpeg", 16), True), ((20, 22, "420mpeg2", 10), False),
                                             ((11, 11, "mono", 8), True), ((17, 33, "444", 12), True)):
        a, b = frames(H, W, chroma, depth)
        code = ref.CHROMAS.index(chroma)
        nb = ref.frame_bytes(H, W, chroma, depth)
        lo = 1 if with_prev else 0
        ins = [guarded.guarded_copy(dev(a[lo:])), guarded.guarded_copy(dev(b[lo:]))]
        prevs = [guarded.guarded_copy(dev(a[0])), guarded.guarded_copy(dev(b[0]))] if with_prev else [None, None]
        n = B - lo
        nbytes = lib.cfen_plane_metrics_bytes(n, H, W, code)
        assert nbytes > 0 and nbytes % 24 == 0
        scratch = guarded.guarded_empty((nbytes,), torch.uint8, DEV)
        out = guarded.guarded_empty((n, 3, 4), torch.int64, DEV)
        full = ref.words(a, b, H, W, chroma, depth)
        wanted = tuple(w[lo:] for w in full) if with_prev else full
        seen = []
        for fill in guarded.FILLS:
            guarded.refill(scratch, fill)
            guarded.refill(out, fill)
            _lib.check(lib.cfen_plane_metrics(_lib.ptr(ins[0]), nb, _lib.ptr(ins[1]), nb, _lib.ptr(prevs[0]), _lib.ptr(prevs[1]), n, H, W, code, depth,
                                              _lib.ptr(scratch), _lib.ptr(out), _lib.current_stream()), "plane_metrics")
            torch.cuda.synchronize()
            guarded.check_bands(scratch, out, *ins, *[p for p in prevs if p is not None])
            words = out.cpu().numpy()
            assert all(np.array_equal(words[:, :, k], wanted[j]) for k, j in ((0, 0), (1, 1), (3, 3))), (H, W, chroma, depth, fill)
            seen.append(out.clone())
        # every bit -- the SSIM's too, which test_words holds to float64 -- is what the call outside the bands gives, whatever the prefill
        plain = _bits(run(dev(a[lo:]), dev(b[lo:]), H, W, chroma, depth, prev=(dev(a[0]), dev(b[0])) if with_prev else None))
        assert all(torch.equal(s.cpu(), plain) for s in seen), (H, W, chroma, depth)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    H, W, chroma, depth = 22, 23, "420jpeg", 10
    a, b = frames(H, W, chroma, depth)
    ta, tb = dev(a), dev(b)
    nb = ref.frame_bytes(H, W, chroma, depth)
    with pytest.raises(ValueError, match="plane_metrics: depth"):
        run(ta, tb, H, W, chroma, 7)
    with pytest.raises(ValueError, match="plane_metrics: depth"):
        run(ta, tb, H, W, chroma, 17)
    with pytest.raises(ValueError, match="chroma must be one of"):
        run(ta, tb, H, W, "411", depth)
    with pytest.raises(ValueError, match=r"plane_metrics \(a\): frames must be"):
        run(ta[:, :-2], tb, H, W, chroma, depth)
    with pytest.raises(ValueError, match=r"plane_metrics \(b\): frames must be"):
        run(ta, tb.float(), H, W, chroma, depth)
    with pytest.raises(ValueError, match="a holds 3 frames"):
        run(ta, tb[:2], H, W, chroma, depth)
    with pytest.raises(ValueError, match="needs prev"):
        run(ta, tb, H, W, chroma, depth, prev=(ta[0], tb[0][:-2]))
    with pytest.raises(ValueError, match="plane_metrics: H"):
        run(ta, tb, 0, W, chroma, depth)
    lib = _lib.load()
    code = ref.CHROMAS.index(chroma)
    out = torch.full((B, 3, 4), 7, dtype=torch.int64, device=DEV)
    scratch = torch.full((lib.cfen_plane_metrics_bytes(B, H, W, code) // 8,), 7, dtype=torch.int64, device=DEV)
    z = _lib.c_void_p(0)
    P = _lib.ptr
    good = dict(a=P(ta), stride_a=nb, b=P(tb), stride_b=nb, a_prev=z, b_prev=z, B=B, H=H, W=W, chroma=code, depth=depth, scratch=P(scratch), out=P(out))

    def raw(**kw):
        v = dict(good, **kw)
        return lib.cfen_plane_metrics(v["a"], v["stride_a"], v["b"], v["stride_b"], v["a_prev"], v["b_prev"], v["B"], v["H"], v["W"], v["chroma"],
                                      v["depth"], v["scratch"], v["out"], _lib.current_stream())

    off = lambda t, k: _lib.c_void_p(t.data_ptr() + k)
    for bad in (dict(a=z), dict(b=z), dict(scratch=z), dict(out=z), dict(a_prev=P(ta)), dict(b_prev=P(tb)), dict(B=0), dict(B=65536), dict(H=0), dict(W=0),
                dict(H=65537), dict(W=65537), dict(H=65536, W=32769, stride_a=1 << 40, stride_b=1 << 40), dict(chroma=5), dict(chroma=-1), dict(depth=7),
                dict(depth=17), dict(stride_a=nb - 2), dict(stride_b=nb - 2), dict(a=off(ta, 1)), dict(b=off(tb, 1)), dict(stride_a=nb + 1),
                dict(stride_b=nb + 1), dict(a_prev=off(ta, 1), b_prev=P(tb)), dict(a_prev=P(ta), b_prev=off(tb, 1)), dict(out=off(out, 4)),
                dict(scratch=off(scratch, 4))):
        assert raw(**bad) == -1 and b"plane_metrics" in lib.cfen_last_error(), bad
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((scratch == 7).all())
    assert raw() == 0                                             # and the same call with nothing wrong runs
    torch.cuda.synchronize()
    got = (out[:, :, 0], out[:, :, 1], out[:, :, 2].contiguous().view(torch.float64), out[:, :, 3])
    check(got, want(H, W, chroma, depth), depth, (H, W, chroma, depth, "raw"))
