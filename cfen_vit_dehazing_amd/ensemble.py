"""Geometric self-ensemble (x8): the generator's output as the mean over the eight flips / transposes of its input.

The reference carries the flag (options/base_options.py:133, --self_ensemble) and the algorithm (models/vit_model.py:102-147, Model.forward_x8,
inherited from IPT) but its dehazing model never joins the two.  This generator is not equivariant under the eight transforms (learned positional
tables, window partition), so the eight forwards differ and their mean is a different, smoother estimate.

Semantics, with v = flip W, h = flip H, t = swap H and W, per T x T plane:
  variant i = b0 + 2 b1 + 4 b2        x_i = t^b2(h^b1(v^b0(x)))                      (v applied first)
  every output plane y_i of net(x_i)  z_i = v^b0(h^b1(t^b2(y_i)))                    (mapped back)
  result                              0.125f * (((((((z_0 + z_1) + z_2) + z_3) + z_4) + z_5) + z_6) + z_7)   in fp32, nothing else

`dehaze_x8` runs one batch-8 forward per image -- the eight variants of an image are one batch of the launch plan the project is tuned around --
each writing its [xr | xs | xd] outputs into its slab of one arena (cfen_x8_expand in front), and one cfen_x8_merge turns the arena into the
results.  Images must be T x T, T = cfg.image_size; other sizes go through tiled.dehaze_tiled(..., self_ensemble=True).
"""
import torch

from . import ops
from ._lib import CfenError

VARIANTS = 8


def actnorm_pending(net):
    """does `net` (a hipnet.dec_ipt) still hold ActNorm layers that its next eager forward would initialise from its batch?"""
    return net.actnorm_pending()


def dehaze_x8(net, images, out=None, output_u8=False, arena=None):
    """[xr (M,3,T,T), xs (M,1,T,T), xd (M,3,T,T)] float32 of the self-ensemble of `net` (a hipnet.dec_ipt) over `images`: (M,T,T,3) uint8 or
    (M,3,T,T) float32 in [-1,1] CUDA tensor, T = net.cfg.image_size.  With output_u8 three (M,T,T,3) uint8 images instead (util.tensor2im's bytes,
    produced by the merge from the float values).  `out`: optional flat float32 buffer of 7*M*T*T elements that receives [xr | xs | xd] back to back
    (the layout of net(x, out=)); the results are views of it.  `arena`: optional flat contiguous buffer of 56*M*T*T elements (float16 for an
    output_f16 net, else float32) the eight forwards' outputs go through; its contents before the call do not matter.

    A net whose ActNorm layers are uninitialised is refused: they would be initialised from the eight variants of the first image, not from a batch
    of the data as the reference's first call does -- run one plain forward of the first batch first."""
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        raise ValueError("dehaze_x8 needs a CUDA tensor; there is no CPU fallback")
    T = net.cfg.image_size
    u8 = images.dtype == torch.uint8
    want = (T, T, 3) if u8 else (3, T, T)
    if images.dim() != 4 or tuple(images.shape[1:]) != want or images.dtype not in (torch.uint8, torch.float32) or images.shape[0] < 1:
        raise ValueError("dehaze_x8 needs (M,%d,%d,3) uint8 or (M,3,%d,%d) float32 images (the generator's image size; other sizes go through "
                         "dehaze_tiled(..., self_ensemble=True)), got %s %s" % (T, T, T, T, tuple(images.shape), images.dtype))
    if actnorm_pending(net):
        raise CfenError("self-ensemble: ActNorm2d layers are uninitialised; run one plain forward of the first batch (it initialises them from that "
                        "batch, models/actnorm.py:25-37) before forward_x8")
    images = images.contiguous()
    M = images.shape[0]
    odt = torch.float16 if net.output_f16 else torch.float32
    slab = 7 * VARIANTS * T * T
    if arena is None:
        arena = torch.empty(M * slab, dtype=odt, device=images.device)
    elif not isinstance(arena, torch.Tensor) or arena.dim() != 1 or arena.numel() != M * slab or arena.dtype != odt or arena.device != images.device \
            or not arena.is_contiguous():
        raise ValueError("dehaze_x8: arena must be a flat contiguous %s buffer of %d elements on the images' device" % (odt, M * slab))
    slab_in = torch.empty((VARIANTS, T, T, 3) if u8 else (VARIANTS, 3, T, T), dtype=images.dtype, device=images.device)
    keep_u8 = net.output_u8
    net.output_u8 = False              # the merge works on the float outputs; bytes come out of the merge
    try:
        for m in range(M):
            ops.x8_expand(images, m, out=slab_in)
            net(slab_in, out=arena[m * slab:(m + 1) * slab])
    finally:
        net.output_u8 = keep_u8
    return ops.x8_merge(arena, M, T, output_u8=output_u8, out=out)
