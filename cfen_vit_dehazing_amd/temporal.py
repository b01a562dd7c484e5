"""Temporal stabilisation of a dehazed stream (include/cfen_temporal.h states the definition).

The generator dehazes every frame on its own, and a small change of the input changes its estimate of airlight and transmission: the output
shimmers.  A Stabiliser fits, per frame, the local affine model out ~ a * hazy + b of guided upsampling (ops.guided_coef_u8) at a working
resolution, smooths (a, b) over time by a recursion that a motion test switches off where the scene changed (ops.temporal_blend), and corrects
the full-resolution output by the CHANGE of the coefficients (ops.temporal_apply_u8): the network's own detail stays, and where nothing is
smoothed the bytes are the network's.  With mc_range > 0 the recursion follows the scene (include/cfen_motion.h): each
block of the working-resolution frame is looked up in the previous frame (ops.motion_search_u8), and the state and the previous frame are
fetched from there (ops.motion_warp) before the same blend runs.  With mc_subpel 2 or 4 the vectors are refined to half or quarter pixels
(ops.motion_refine_u8) and the fetch is bilinear (ops.motion_warp_subpel; include/cfen_subpel.h): the working resolution is
1 / down of the frame, so a real pan is a fraction of a working pixel.  Everything runs on the current stream; nothing synchronises with the host."""
import math

import torch

from . import ops

DEFAULTS = {"radius": 2, "eps": 1e-4, "strength": 0.8, "motion": 8.0, "down": "auto"}


def check_params(radius, eps, strength, motion, down, what="Stabiliser"):
    """(radius, eps, strength, motion, down) as int, float, float, float, int or 'auto'; ValueError naming the argument out of range"""
    try:
        r, e, s, m = int(radius), float(eps), float(strength), float(motion)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("%s: radius must be an integer, eps, strength and motion numbers, got %r, %r, %r, %r" % (what, radius, eps, strength, motion))
    if r != radius or not 1 <= r <= 16:
        raise ValueError("%s: radius must be an integer in 1 .. 16, got %r" % (what, radius))
    if not (math.isfinite(e) and e > 0):
        raise ValueError("%s: eps must be finite and > 0, got %r" % (what, eps))
    if not 0 <= s < 1:
        raise ValueError("%s: strength must be in [0, 1), got %r" % (what, strength))
    if not (math.isfinite(m) and m > 0):
        raise ValueError("%s: motion must be finite and > 0, got %r" % (what, motion))
    if down != "auto":
        try:
            d = int(down)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("%s: down must be 'auto' or an integer >= 1, got %r" % (what, down))
        if d != down or d < 1:
            raise ValueError("%s: down must be 'auto' or an integer >= 1, got %r" % (what, down))
        down = d
    return r, e, s, m, down


# motion compensation: range 0 = off; block and bias from the synthetic panning experiment of DESIGN section 20
MC_DEFAULTS = {"range": 0, "block": 16, "bias": 4}


def check_mc_params(mc_range, mc_block, mc_bias, what="Stabiliser"):
    """(mc_range, mc_block, mc_bias) as ints; ValueError naming the argument out of range"""
    out = []
    for name, v, ok, say in (("mc_range", mc_range, lambda i: 0 <= i <= 16, "an integer in 0 .. 16 (0 = off)"),
                             ("mc_block", mc_block, lambda i: i in (8, 16, 32), "8, 16 or 32"),
                             ("mc_bias", mc_bias, lambda i: 0 <= i <= 255, "an integer in 0 .. 255")):
        try:
            i = int(v)
        except (TypeError, ValueError, OverflowError):
            i = None
        if i is None or i != v or not ok(i):
            raise ValueError("%s: %s must be %s, got %r" % (what, name, say, v))
        out.append(i)
    return tuple(out)


# sub-pixel refinement of the block vectors (include/cfen_subpel.h): 1 = whole pixels, the path without; 2 and 4 = half and quarter pixels
MC_SUBPEL = (1, 2, 4)


def check_mc_subpel(mc_subpel, mc_range=None, what="Stabiliser"):
    """mc_subpel as an int; ValueError unless it is 1, 2 or 4, and -- where mc_range is given -- unless refinement has vectors to refine"""
    try:
        i = int(mc_subpel)
    except (TypeError, ValueError, OverflowError):
        i = None
    if i is None or i != mc_subpel or i not in MC_SUBPEL:
        raise ValueError("%s: mc_subpel must be 1, 2 or 4, got %r" % (what, mc_subpel))
    if i > 1 and mc_range is not None and not mc_range:
        raise ValueError("%s: mc_subpel = %d refines the vectors of motion compensation: it needs mc_range > 0" % (what, i))
    return i


def working_size(H, W, down="auto"):
    """(S, h, w): the factor and the working resolution of H x W frames; auto is S = ceil(max(H, W) / 1024)"""
    S = -(-max(H, W) // 1024) if down == "auto" else int(down)
    return S, -(-H // S), -(-W // S)


class Stabiliser:
    """step(hazy_u8, out_u8) for consecutive batches of consecutive frames, (n,H,W,3) uint8 CUDA tensors: the stabilised (n,H,W,3) uint8 frames.
    The first frame after construction or reset() passes unchanged.  The object owns the recursion's state, a copy of the last working-resolution
    hazy frame and its scratch tensors; the result does not depend on how the frames are grouped into batches.  mc_range > 0 (keyword only, with
    mc_block and mc_bias): motion compensation, one search launch per batch and a warp and a one-frame blend per frame; 0 is the path without.
    mc_subpel 2 or 4 (keyword only, needs mc_range > 0): one refine launch per batch after the search, and the sub-pixel warp; 1 is the path
    without."""

    def __init__(self, radius=2, eps=1e-4, strength=0.8, motion=8.0, down="auto", *, mc_range=MC_DEFAULTS["range"], mc_block=MC_DEFAULTS["block"],
                 mc_bias=MC_DEFAULTS["bias"], mc_subpel=MC_SUBPEL[0]):
        self.radius, self.eps, self.strength, self.motion, self.down = check_params(radius, eps, strength, motion, down)
        self.mc_range, self.mc_block, self.mc_bias = check_mc_params(mc_range, mc_block, mc_bias)
        self.mc_subpel = check_mc_subpel(mc_subpel, self.mc_range)
        self.reset()

    def reset(self):
        """the next frame is the first of a stream (frames of another size may follow)"""
        self._have = False
        self._key = None
        self._state = self._prev = self._coef = self._delta = None
        self._state2 = self._warped = self._vec = self._sad = self._frame = None          # motion compensation: the second state, I^w, the batch's field
        self._vec4 = self._sad4 = None                                                     # the batch's refined field

    def step(self, hazy_u8, out_u8, out=None):
        for name, t in (("hazy_u8", hazy_u8), ("out_u8", out_u8)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 3 or t.dtype != torch.uint8 or min(t.shape) < 1 or not t.is_cuda or \
                    not t.is_contiguous():
                raise ValueError("Stabiliser.step needs %s as a contiguous (n,H,W,3) uint8 CUDA tensor, got %s"
                                 % (name, "%s %s" % (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__))
        if hazy_u8.shape != out_u8.shape or hazy_u8.device != out_u8.device:
            raise ValueError("Stabiliser.step: hazy_u8 %s and out_u8 %s differ in shape or device" % (tuple(hazy_u8.shape), tuple(out_u8.shape)))
        n, H, W, _ = hazy_u8.shape
        dev = hazy_u8.device
        key = (H, W, dev)
        if self._key is not None and key != self._key:
            raise ValueError("Stabiliser.step: frames of %d x %d on %s after frames of %d x %d on %s: reset() starts a new stream"
                             % (H, W, dev, self._key[0], self._key[1], self._key[2]))
        S, h, w = working_size(H, W, self.down)
        if self._key is None:
            self._key = key
            self._state = torch.empty(h, w, 6, dtype=torch.float32, device=dev)
            self._prev = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        if self._coef is None or self._coef.shape[0] < n:
            self._coef = torch.empty(n, h, w, 6, dtype=torch.float32, device=dev)
            self._delta = torch.empty(n, h, w, 6, dtype=torch.float32, device=dev)
        if S == 1:
            I, P = hazy_u8, out_u8
        else:
            I, P = ops.resample_u8(hazy_u8, (h, w), filter="box"), ops.resample_u8(out_u8, (h, w), filter="box")
        coef = ops.guided_coef_u8(I, P, self.radius, self.eps, out=self._coef[:n])
        if self.mc_range:
            delta = self._blend_compensated(I, coef, n)
        else:
            delta = ops.temporal_blend(I, self._prev, coef, self._state, self.radius, self.motion, self.strength, self._have, out=self._delta[:n])
        self._prev.copy_(I[n - 1])                 # after the launch that read it, on the same stream
        self._have = True
        return ops.temporal_apply_u8(delta, hazy_u8, out_u8, out=out)

    def _blend_compensated(self, I, coef, n):
        """the compensated recursion of include/cfen_motion.h over the n frames I: one search for the batch, then per frame the warp into the
        other state buffer and the one-frame blend on it, in place.  mc_subpel > 1: the recursion of include/cfen_subpel.h, one refine after the
        search and the sub-pixel warp in place of the warp"""
        _, h, w, _ = I.shape
        bh, bw = -(-h // self.mc_block), -(-w // self.mc_block)
        if self._state2 is None:
            self._state2 = torch.empty_like(self._state)
            self._warped = torch.empty_like(self._prev)
        if self._vec is None or self._vec.shape[0] < n:
            self._vec = torch.empty(n, bh, bw, 2, dtype=torch.int16, device=I.device)
            self._sad = torch.empty(n, bh, bw, dtype=torch.int32, device=I.device)
        if self.mc_subpel > 1 and (self._vec4 is None or self._vec4.shape[0] < n):
            self._vec4 = torch.empty(n, bh, bw, 2, dtype=torch.int16, device=I.device)
            self._sad4 = torch.empty(n, bh, bw, dtype=torch.int32, device=I.device)
        delta = self._delta[:n]
        first = 0 if self._have else 1                     # the first frame of a stream has no predecessor to search
        if not self._have:
            ops.temporal_blend(I[:1], None, coef[:1], self._state, self.radius, self.motion, self.strength, False, out=delta[:1])
        if first < n:
            vec, _ = ops.motion_search_u8(I[first:], I[0] if first else self._prev, self.mc_block, self.mc_range, self.mc_bias,
                                          out=(self._vec[:n - first], self._sad[:n - first]))
            if self.mc_subpel > 1:
                vec, _ = ops.motion_refine_u8(I[first:], I[0] if first else self._prev, vec, self.mc_block, self.mc_subpel, self.mc_bias,
                                              out=(self._vec4[:n - first], self._sad4[:n - first]))
        warp = ops.motion_warp_subpel if self.mc_subpel > 1 else ops.motion_warp
        for k in range(first, n):
            warp(vec[k - first], I[k - 1] if k else self._prev, self._state, self.mc_block, out=(self._warped, self._state2))
            ck, dk = coef[k:k + 1], delta[k:k + 1]
            aside = bool((k * h * w) % 2)                  # 24 k h w bytes into the batch: not the 16-byte boundary the blend asks for
            if aside:
                if self._frame is None:
                    self._frame = (torch.empty_like(ck), torch.empty_like(dk))
                ck, dk = self._frame[0].copy_(ck), self._frame[1]
            ops.temporal_blend(I[k:k + 1], self._warped, ck, self._state2, self.radius, self.motion, self.strength, True, out=dk)
            if aside:
                delta[k:k + 1].copy_(dk)
            self._state, self._state2 = self._state2, self._state
        return delta
