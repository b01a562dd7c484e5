#!/usr/bin/env python3
"""Writes tests/golden/image_parity.npz: what the image-side entry points (guided, temporal, PSNR / SSIM, MS-SSIM, CIEDE2000, no-reference
statistics, PNG) give, bit for bit, for the smallest inputs that reach each of their paths.

    CFEN_HIP_LIB=<libcfen_hip.so of the commit to pin> PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_image_parity.py

Needs a GPU.  It calls the entry points through whatever library cfen_vit_dehazing_amd._lib loads, on inputs made by the seeded generators of
tests/, and writes only the outputs.  The committed fixture was written ONCE, with the library built from the commit before these kernels' shared
code moved into csrc/cfen_image.hpp; tests/test_hip_image_parity.py holds the current library to it with no tolerance.  A refactor of these kernels
does not regenerate it: that is the point of it.

CASES maps a case's name to a function that returns {output name: numpy array}; the test runs the same functions.  An output of more than
WHOLE_BYTES bytes is stored as the SHA-256 of its dtype, shape and bytes (`packed`), so that the fixture stays a small file: equality of the digests
is equality of the bits."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
sys.dont_write_bytecode = True

import torch  # noqa: E402

import guided_ref  # noqa: E402
import metrics_images as mi  # noqa: E402
import noref_ref  # noqa: E402
import png_ref  # noqa: E402
import temporal_ref  # noqa: E402
from cfen_vit_dehazing_amd import ops  # noqa: E402

DEV = "cuda:0"
FIXTURE = os.path.join(ROOT, "tests", "golden", "image_parity.npz")
WHOLE_BYTES = 4096


def packed(a):
    """what the fixture holds of an output: the array itself, or its digest as 32 bytes"""
    a = np.ascontiguousarray(a)
    if a.nbytes <= WHOLE_BYTES:
        return a
    h = hashlib.sha256(("%s %s " % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                 # a copy: the shared case arrays are read-only


def host(**tensors):
    return {k: v.cpu().numpy() for k, v in tensors.items()}


# ---- guided -------------------------------------------------------------------------------------------------------------------------------------
def guided_coef(name, eps):
    I, P = guided_ref.coef_case(name, "model", eps)[:2]
    return host(coef=ops.guided_coef_u8(dev(I), dev(P), guided_ref.COEF_CASES[name][3], eps))


def guided_apply(name):
    G, I, P = guided_ref.apply_case(name)[:3]
    coef = ops.guided_coef_u8(dev(I), dev(P), guided_ref.APPLY_CASES[name][2], 1e-4)
    return host(coef=coef, dst=ops.guided_apply_u8(coef, dev(G)))


# ---- temporal -----------------------------------------------------------------------------------------------------------------------------------
def temporal_blend(h, w, r, have_state):
    guide, prev, coef, state0 = temporal_ref.blend_case(h, w, r, 3, have_state)[:4]
    state = dev(state0) if have_state else torch.full((h, w, 6), float("nan"), device=DEV)
    delta = ops.temporal_blend(dev(guide), dev(prev) if have_state else None, dev(coef), state, r, temporal_ref.MOTION, temporal_ref.STRENGTH,
                               have_state)
    return host(delta=delta, state=state)


def temporal_apply(name, offset=0):
    """offset: where in a larger slab dst begins -- 0 takes the 16-byte path where the row pitch allows it, 1 the byte path on the same data"""
    delta, G, Y = temporal_ref.apply_case(name)[:3]
    slab = torch.zeros(G.size + 16, dtype=torch.uint8, device=DEV)
    dst = slab[offset:offset + G.size].view(G.shape)
    ops.temporal_apply_u8(dev(delta), dev(G), dev(Y), out=dst)
    return host(dst=dst)


# ---- scores against ground truth ----------------------------------------------------------------------------------------------------------------
def noisy_pair(B, H, W, seed):
    """(a, b) (B,H,W,3) uint8: b blocks of 8 with fine noise, a = b with a veil and more noise"""
    rs = np.random.RandomState(seed)
    b = np.clip(np.kron(rs.randint(0, 256, (B, -(-H // 8), -(-W // 8), 3)), np.ones((1, 8, 8, 1), dtype=np.int64))[:, :H, :W] +
                rs.randint(-6, 7, (B, H, W, 3)), 0, 255)
    a = np.clip(b * 3 // 4 + 50 + rs.randint(-10, 11, (B, H, W, 3)), 0, 255)
    return a.astype(np.uint8), b.astype(np.uint8)


def metrics(a, b, f32):
    if f32:
        a, b = (np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255) for x in (a, b))
    sse, ssim = ops.image_metrics(dev(a), dev(b), value_range=(0.0, 1.0))
    return host(sse=sse, ssim=ssim)


def msssim(H, W, seed):
    sse, levels = ops.image_msssim(*(dev(x) for x in noisy_pair(1, H, W, seed)))
    return host(sse=sse, levels=levels)


def ciede(shape, seed):
    a, b = (dev(x) for x in noisy_pair(*shape, seed))
    with_map, dmap = ops.image_ciede2000(a, b, map=True)
    return host(mean=ops.image_ciede2000(a, b), mean_with_map=with_map, map=dmap)


def noref(name):
    hazy, out, r = noref_ref.case(name)[:3]
    counts, grad = ops.image_noref(dev(hazy), dev(out), r)
    counts_m, grad_m, d0, d1 = ops.image_noref(dev(hazy), dev(out), r, maps=True)
    return host(counts=counts, grad=grad, counts_with_maps=counts_m, grad_with_maps=grad_m, dark_hazy=d0, dark_out=d1)


def png():
    slab, lengths = ops.png_deflate(dev(np.stack([png_ref.smooth(37, 53, 11), png_ref.smooth(37, 53, 12)])))
    slab, lengths = slab.cpu().numpy(), lengths.cpu().numpy()
    return {"lengths": lengths, "streams": np.concatenate([slab[i, :lengths[i]] for i in range(len(lengths))])}


CASES = {}
for _n in guided_ref.COEF_CASES:
    for _e in guided_ref.EPS:
        CASES["guided_coef/%s/eps%g" % (_n, _e)] = lambda n=_n, e=_e: guided_coef(n, e)
for _n in guided_ref.APPLY_CASES:
    CASES["guided_apply/" + _n] = lambda n=_n: guided_apply(n)
for _h, _w in temporal_ref.SIZES:
    for _r in temporal_ref.RADII:
        for _s in (False, True):
            CASES["temporal_blend/%dx%d_r%d_%s" % (_h, _w, _r, "carried" if _s else "first")] = lambda h=_h, w=_w, r=_r, s=_s: temporal_blend(h, w, r, s)
for _n in temporal_ref.APPLY_CASES:
    CASES["temporal_apply/" + _n] = lambda n=_n: temporal_apply(n)
CASES["temporal_apply/40x32_1to1_offset1"] = lambda: temporal_apply("40x32_1to1", 1)
for _n in ("11x11", "37x53"):
    for _f in (False, True):
        CASES["metrics/%s_%s" % (_n, "f32" if _f else "u8")] = lambda n=_n, f=_f: metrics(*mi.pair(n), f)
CASES["metrics/418x1034_u8"] = lambda: metrics(*noisy_pair(1, 418, 1034, 21), False)      # 17 x 16 = 272 tiles: the finish loop runs twice
CASES["msssim/176x176"] = lambda: msssim(176, 176, 22)
CASES["msssim/200x333"] = lambda: msssim(200, 333, 23)
for _s in ((1, 1, 1), (3, 17, 67), (1, 513, 512)):                                           # one pixel; misaligned image starts; 257 partials
    CASES["ciede2000/%dx%dx%d" % _s] = lambda s=_s: ciede(s, 24 + s[1])
for _n in ("1x1x1_r7", "2x3x5_r7", "3x17x67_r7"):
    CASES["noref/" + _n] = lambda n=_n: noref(n)
CASES["png/2x37x53"] = png


def main():
    out = {}
    for name, fn in CASES.items():
        for k, v in fn().items():
            out[name + "/" + k] = packed(v)
        print(name, flush=True)
    np.savez_compressed(FIXTURE, **out)
    print("%d outputs of %d cases -> %s (%d bytes)" % (len(out), len(CASES), FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
