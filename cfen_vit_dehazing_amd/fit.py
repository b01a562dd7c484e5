"""Fit-to-size inference: an image of any size is resampled to the generator's T x T (T = cfg.image_size is baked into the checkpoint), run through
ONE unchanged forward, and every output is resampled back to the image's size.  Unlike tiled.py the network sees the whole scene -- what its GViT
branch is for -- at the price of the resampling loss (refine="guided" gives the dehazed image its full-resolution detail back, below).  The aspect ratio is NOT kept: this is PIL's Image.resize((T, T)) and Image.resize((W, H)).

Both resamples are PIL's 8-bit fixed-point algorithm on the device (ops.resample_u8, csrc/k_resample.hip; tables from resample.py), byte for byte
what `Image.resize(..., Image.BICUBIC)` around test.py would give -- the reference's own choice wherever it resizes (data/base_dataset.py
get_transform).  A T x T image skips both and is bitwise the plain forward.

refine="guided": the dehazed output xd is not stretched back with the filter but upsampled with the hazy image as a guide (ops.guided_upsample_u8,
csrc/k_guided.hip, include/cfen_guided.h: He & Sun's fast guided filter).  Under the scattering model I = J t + A (1 - t) the clear image is
locally affine in I per channel wherever the transmission is smooth, so a linear model xd ~ a x + b fitted per pixel at T x T between the bytes the
forward was fed and its output, smoothed, upsampled bilinearly and applied to the FULL-resolution image carries the network's low frequencies and
the input's detail.  xr and xs keep the plain resample: shading is one channel repeated three times (a per-channel guide would colour it), and
reflectance is not the image that is kept or scored.
"""
import torch

from . import ops

_LUT = {}


def normalize_u8(images_u8):
    """(B,T,T,3) uint8 -> (B,3,T,T) float32 with data.to_normalized_tensor's fp32 arithmetic: its 256 results, computed once on the host by that
    very expression, looked up per byte"""
    dev = images_u8.device
    key = (dev.type, dev.index)
    if key not in _LUT:
        _LUT[key] = ((torch.arange(256, dtype=torch.uint8).float().div(255.0) - 0.5) / 0.5).to(dev)
    return _LUT[key][images_u8.permute(0, 3, 1, 2).long()].contiguous()


def _check_image(t, what):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or t.shape[-1] != 3 or min(t.shape) < 1:
        raise ValueError("forward_fit needs %s uint8 CUDA tensor(s) as decoded from the file; there is no CPU fallback (got %s)"
                         % (what, "%s %s on %s" % (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t).__name__))


def _forward_u8(net, x, self_ensemble):
    """[xr, xs, xd] (B,T,T,3) uint8 of the unchanged forward: native uint8 outputs where the plan has them, the tensor2im_u8 pass elsewhere"""
    if self_ensemble:
        return net.forward_x8(x, output_u8=True)
    keep = net.output_u8
    net.output_u8 = True
    try:
        return net(x)
    finally:
        net.output_u8 = keep


REFINES = (None, "guided")


def check_refine(refine, radius, eps):
    """refuse what ops.guided_upsample_u8 would refuse, before the forward runs"""
    if refine not in REFINES:
        raise ValueError("forward_fit: refine must be None or 'guided', got %r" % (refine,))
    if refine is not None:
        ops._guided_params("forward_fit", radius, eps)


def back_to_size(outs_lo, x, image, filter, refine=None, radius=2, eps=1e-4):
    """[xr, xs, xd] (B,T,T,3) uint8 of the forward -> the three at the size of image (B,H,W,3) uint8, which x (B,T,T,3) is the resampled copy of:
    the filter for all three, or with refine="guided" the guided upsampling for xd"""
    size = image.shape[1:3]
    outs = [ops.resample_u8(o, size, filter) for o in (outs_lo[:2] if refine else outs_lo)]
    if refine:
        outs.append(ops.guided_upsample_u8(image, x, outs_lo[2], radius, eps))
    return outs


def dehaze_fit(net, images, filter="bicubic", self_ensemble=False, u8_input=True, refine=None, radius=2, eps=1e-4):
    """[xr, xs, xd] of `net` (a hipnet.dec_ipt), each uint8 at the size of the input (xs repeated to three channels, as in the u8 output mode).

    images: a (B,H,W,3) uint8 CUDA tensor -> three (B,H,W,3) tensors; or a list of (H_i,W_i,3) uint8 CUDA tensors of any sizes, which run as ONE
    batch (every image resampled into its lane of the input slab, every output lane resampled back to its image's size) -> three lists of
    (H_i,W_i,3) tensors.  filter: one of resample.FILTERS.  self_ensemble: the forward is forward_x8.  u8_input: the bytes go to a uint8-input
    net as they are; False normalises them to (B,3,T,T) float32 first (normalize_u8) for a float-input net -- the same results.
    refine: None, or "guided": xd of a resized image is ops.guided_upsample_u8(image, x, xd at T x T, radius, eps) with x the T x T bytes that went
    into the forward, instead of the resampled xd; xr and xs keep the plain resample."""
    check_refine(refine, radius, eps)
    T = net.cfg.image_size
    many = isinstance(images, (list, tuple))
    if many:
        if not images:
            raise ValueError("forward_fit: empty list of images")
        for t in images:
            _check_image(t, "(H,W,3)")
            if t.dim() != 3:
                raise ValueError("forward_fit: a list holds (H,W,3) images, got %s" % (tuple(t.shape),))
        x = torch.empty(len(images), T, T, 3, dtype=torch.uint8, device=images[0].device)
        for i, t in enumerate(images):
            if tuple(t.shape[:2]) == (T, T):
                x[i].copy_(t)
            else:
                ops.resample_u8(t.contiguous()[None], (T, T), filter, out=x[i:i + 1])
    else:
        _check_image(images, "a (B,H,W,3)")
        if images.dim() != 4:
            raise ValueError("forward_fit needs a (B,H,W,3) uint8 tensor or a list of (H,W,3) tensors, got %s" % (tuple(images.shape),))
        images = images.contiguous()
        x = images if tuple(images.shape[1:3]) == (T, T) else ops.resample_u8(images, (T, T), filter)
    outs = _forward_u8(net, x if u8_input else normalize_u8(x), self_ensemble)
    if not many:
        H, W = images.shape[1:3]
        return list(outs) if (H, W) == (T, T) else back_to_size([o.contiguous() for o in outs], x, images, filter, refine, radius, eps)
    if not refine:
        return [[o[i] if tuple(t.shape[:2]) == (T, T) else ops.resample_u8(o[i:i + 1], t.shape[:2], filter)[0] for i, t in enumerate(images)] for o in outs]
    lanes = [[o[i:i + 1] for o in outs] if tuple(t.shape[:2]) == (T, T) else
             back_to_size([o[i:i + 1].contiguous() for o in outs], x[i:i + 1], t.contiguous()[None], filter, refine, radius, eps) for i, t in enumerate(images)]
    return [[lane[k][0] for lane in lanes] for k in range(3)]
