"""Dehaze images of any size with the fixed-size generator: overlapping T x T tiles, T = cfg.image_size.

The generator's image size is baked in (learned positional tables and F.fold(..., img_dim): reference v3:1125-1127, 1186, 1321), so
`dec_ipt` refuses anything but T x T.  `dehaze_tiled` cuts an H x W image into overlapping tiles (cfen_tile_gather), runs them through the
unchanged forward in batches, each batch writing its [xr | xs | xd] outputs straight into its slab of one tile arena, and blends the arena back
into full-size outputs (cfen_tile_blend).

Tile plan, per axis of extent L, overlap o (0 <= o <= T/2, default T // 8):
  n   = 1 if L <= T else 1 + ceil((L - T) / (T - o))
  p_j = (j * (L - T)) // (n - 1) for n > 1, else p_0 = 0       (evenly spread, the last tile flush with the far edge)
  tile pixel (u, v) of tile (i, j), t = i * nx + j, reads source pixel (mirror(p_i + u, H), mirror(q_j + v, W)); mirror = numpy 'reflect'
  weight w(u) = min(1, (min(u, e - 1 - u) + 1) / (o + 1)), e = min(T, L); a tile's weight is w_y * w_x
  output = the tile value where exactly one tile covers the pixel, else sum(w v) / sum(w) in fp32 over the covering tiles in increasing t
"""
import torch

from . import ensemble, ops

MAX_ARENA_BYTES = 8 << 30


def tile_count(L, T, overlap):
    """tiles along an axis of extent L"""
    return 1 if L <= T else 1 + -(-(L - T) // (T - overlap))


def tile_origins(L, T, n):
    return [0] if n == 1 else [(j * (L - T)) // (n - 1) for j in range(n)]


def default_overlap(T):
    return T // 8


def tile_grid(H, W, T, overlap):
    """(row origins, column origins) of the tile plan of an H x W image; ValueError on a bad size or overlap"""
    for name, v in (("H", H), ("W", W), ("T", T), ("overlap", overlap)):
        if not isinstance(v, int) or isinstance(v, bool):
            raise ValueError("tile_grid: %s must be an int, got %r" % (name, v))
    if T < 2:
        raise ValueError("tile_grid: tile edge T = %d must be >= 2" % T)
    if H < 1 or W < 1:
        raise ValueError("tile_grid: image size %d x %d is empty" % (H, W))
    if not 0 <= overlap <= T // 2:
        raise ValueError("tile_grid: overlap %d outside 0 .. T/2 = %d" % (overlap, T // 2))
    return tile_origins(H, T, tile_count(H, T, overlap)), tile_origins(W, T, tile_count(W, T, overlap))


def dehaze_tiled(net, image, overlap=None, tile_batch=8, output_u8=False, max_arena_bytes=MAX_ARENA_BYTES, self_ensemble=False, arena=None):
    """[xr, xs, xd] of an image of any size through `net` (a hipnet.dec_ipt) as overlapping T x T tiles.

    image: (H,W,3) uint8 or (3,H,W) float32 in [-1,1] CUDA tensor; a leading batch dimension of 1 is accepted and kept on the outputs.
    Returns float32 xr (3,H,W), xs (1,H,W), xd (3,H,W), or with output_u8 three (H,W,3) uint8 images (util.tensor2im's bytes, produced by the
    blend from the float values).  Tiles run tile_batch at a time (the last batch padded with copies of the last tile); a net whose ActNorm layers
    are still uninitialised initialises them from the first tile batch, as its first plain forward would.  An image whose single-tile plan covers
    it (H = W = T) comes out bitwise as the plain forward's.  self_ensemble: every tile batch goes through the geometric self-ensemble
    (ensemble.dehaze_x8: eight forwards per tile) into a float32 arena, the blend is the same; the ActNorm layers must be initialised then.
    arena: optional flat contiguous CUDA buffer the tile outputs go through, of exactly ceil(tiles / B) * 7 * B * T * T elements (B = min(tile_batch,
    tiles)), float16 for an output_f16 net without self_ensemble, else float32; its contents before the call do not matter.  Default: allocated here."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda:
        raise ValueError("dehaze_tiled needs a CUDA tensor image; there is no CPU fallback")
    batched = image.dim() == 4
    if batched:
        if image.shape[0] != 1:
            raise ValueError("dehaze_tiled takes one image (a leading batch dimension of 1 at most), got %s" % (tuple(image.shape),))
        image = image[0]
    u8 = image.dtype == torch.uint8
    if image.dim() != 3 or (u8 and image.shape[2] != 3) or (not u8 and (image.dtype != torch.float32 or image.shape[0] != 3)):
        raise ValueError("dehaze_tiled needs an (H,W,3) uint8 or (3,H,W) float32 image, got %s %s" % (tuple(image.shape), image.dtype))
    image = image.contiguous()
    H, W = (image.shape[0], image.shape[1]) if u8 else (image.shape[1], image.shape[2])
    T = net.cfg.image_size
    o = default_overlap(T) if overlap is None else int(overlap)
    ys, xs = tile_grid(H, W, T, o)
    ny, nx = len(ys), len(xs)
    ntiles = ny * nx
    if tile_batch < 1:
        raise ValueError("tile_batch must be >= 1")
    B = min(int(tile_batch), ntiles)
    nslabs = -(-ntiles // B)
    odt = torch.float16 if net.output_f16 and not self_ensemble else torch.float32
    slab = 7 * B * T * T
    arena_bytes = nslabs * slab * (2 if odt == torch.float16 else 4)
    if arena_bytes > max_arena_bytes:
        raise ValueError("a %d x %d image is %d x %d tiles of %d x %d: their outputs need a %.2f GiB arena, over the %.2f GiB limit (max_arena_bytes)"
                         % (H, W, ny, nx, T, T, arena_bytes / 2 ** 30, max_arena_bytes / 2 ** 30))
    if arena is None:
        arena = torch.empty(nslabs * slab, dtype=odt, device=image.device)
    elif not isinstance(arena, torch.Tensor) or arena.dim() != 1 or arena.numel() != nslabs * slab or arena.dtype != odt or arena.device != image.device \
            or not arena.is_contiguous():
        raise ValueError("dehaze_tiled: arena must be a flat contiguous %s buffer of %d elements (%d slabs of 7*%d*%d*%d) on the image's device"
                         % (odt, nslabs * slab, nslabs, B, T, T))
    slab_in = torch.empty((B, T, T, 3) if u8 else (B, 3, T, T), dtype=image.dtype, device=image.device)
    keep_u8 = net.output_u8
    net.output_u8 = False              # the blend works on the float outputs; bytes come out of the blend, never get blended
    try:
        for s in range(nslabs):
            ops.tile_gather(image, T, ny, nx, s * B, B, out=slab_in)
            if self_ensemble:
                ensemble.dehaze_x8(net, slab_in, out=arena[s * slab:(s + 1) * slab])
            else:
                net(slab_in, out=arena[s * slab:(s + 1) * slab])
    finally:
        net.output_u8 = keep_u8
    outs = ops.tile_blend(arena, B, T, H, W, ny, nx, o, output_u8=output_u8)
    return [t[None] for t in outs] if batched else outs
