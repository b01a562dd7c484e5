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

Several images in one call (dehaze_tiled_many): the tiles of a group of images are numbered one after another (pack_plan) -- image k's tile t is
global slot slot0_k + t, slab slot // B, lane slot % B -- so an image may start in the middle of a slab and a slab may hold tiles of several
images.  Each slab is filled by one gather per (image, run of tiles) segment and runs through one batch-B forward; each image is blended from the
slab that holds its tile 0 on, with lane0 = slot0 % B (cfen_tile_blend).  Only the last slab of a group is padded.
"""
import collections

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


PackPlan = collections.namedtuple("PackPlan", "images B nslabs slabs")


def pack_plan(sizes, T, overlap, tile_batch):
    """The slot layout of a group of images whose tiles share batches.  sizes: [(H, W), ...].  Returns PackPlan(images, B, nslabs, slabs):
      images : per image (slot0, ny, nx); slot0 is the running sum of the tile counts in front of it
      B      : min(tile_batch, total tiles), the batch of every forward
      nslabs : ceil(total / B)
      slabs  : per slab the gather segments [(image, t0, count, lane), ...]: tiles [t0, t0 + count) of that image go to lanes [lane, lane + count).
               The last segment of the last slab is extended over the padding lanes (the gather repeats the image's last tile there)."""
    if not isinstance(tile_batch, int) or isinstance(tile_batch, bool) or tile_batch < 1:
        raise ValueError("tile_batch must be an int >= 1")
    sizes = list(sizes)
    if not sizes:
        raise ValueError("pack_plan: no images")
    images, total = [], 0
    for H, W in sizes:
        ys, xs = tile_grid(H, W, T, overlap)
        images.append((total, len(ys), len(xs)))
        total += len(ys) * len(xs)
    B = min(tile_batch, total)
    nslabs = -(-total // B)
    slabs = [[] for _ in range(nslabs)]
    for k, (slot0, ny, nx) in enumerate(images):
        t, n = 0, ny * nx
        while t < n:
            s, lane = divmod(slot0 + t, B)
            count = min(n - t, B - lane)
            slabs[s].append((k, t, count, lane))
            t += count
    k, t0, count, lane = slabs[-1][-1]
    slabs[-1][-1] = (k, t0, B - lane, lane)
    return PackPlan(images, B, nslabs, slabs)


def pack_groups(sizes, T, overlap, tile_batch, elem_bytes, max_arena_bytes=MAX_ARENA_BYTES):
    """Consecutive sub-groups [(first, last + 1), ...] of the images, split at image boundaries so that the arena of each -- nslabs * 7 * B * T * T
    elements of elem_bytes, by its own pack_plan -- stays within max_arena_bytes; greedy, in order.  ValueError when one image alone is over."""
    sizes = list(sizes)

    def arena_bytes(a, b):
        plan = pack_plan(sizes[a:b], T, overlap, tile_batch)
        return plan.nslabs * 7 * plan.B * T * T * elem_bytes

    groups, a = [], 0
    while a < len(sizes):
        if arena_bytes(a, a + 1) > max_arena_bytes:
            H, W = sizes[a]
            ys, xs = tile_grid(H, W, T, overlap)
            raise ValueError("a %d x %d image is %d x %d tiles of %d x %d: their outputs need a %.2f GiB arena, over the %.2f GiB limit (max_arena_bytes)"
                             % (H, W, len(ys), len(xs), T, T, arena_bytes(a, a + 1) / 2 ** 30, max_arena_bytes / 2 ** 30))
        b = a + 1
        while b < len(sizes) and arena_bytes(a, b + 1) <= max_arena_bytes:
            b += 1
        groups.append((a, b))
        a = b
    return groups


def dehaze_tiled_many(net, images, overlap=None, tile_batch=8, output_u8=False, max_arena_bytes=MAX_ARENA_BYTES, self_ensemble=False):
    """[[xr, xs, xd], ...] of a list of images of any sizes through `net`, their tiles packed into common batches (pack_plan): a folder of small
    images runs ceil(total tiles / tile_batch) full forwards instead of one short, padded forward sequence per image.

    images: CUDA tensors, all (H,W,3) uint8 or all (3,H,W) float32 in [-1,1]; the sizes may differ.  Per image the result has the shapes and dtypes
    dehaze_tiled returns, and a list of one image returns what dehaze_tiled returns for it, bit for bit.  One arena and one input slab serve the
    group; a group whose arena would exceed max_arena_bytes is split at image boundaries into consecutive sub-groups (pack_groups).  The ActNorm
    layers must be initialised (ValueError otherwise): a packed first batch is not the batch the data-dependent initialisation of dehaze_tiled or
    of a plain forward would see."""
    images = list(images)
    if not images:
        return []
    for im in images:
        if not isinstance(im, torch.Tensor) or not im.is_cuda:
            raise ValueError("dehaze_tiled_many needs CUDA tensor images; there is no CPU fallback")
    u8 = images[0].dtype == torch.uint8
    for im in images:
        if im.dim() != 3 or im.dtype != images[0].dtype or im.device != images[0].device or (u8 and im.shape[2] != 3) \
                or (not u8 and (im.dtype != torch.float32 or im.shape[0] != 3)):
            raise ValueError("dehaze_tiled_many needs images that are all (H,W,3) uint8 or all (3,H,W) float32 on one device, got %s %s"
                             % (tuple(im.shape), im.dtype))
    if ensemble.actnorm_pending(net):
        raise ValueError("dehaze_tiled_many: ActNorm2d layers are uninitialised; a packed first batch would change what their data-dependent "
                         "initialisation sees -- run the first image through dehaze_tiled (or a plain forward) first")
    images = [im.contiguous() for im in images]
    sizes = [(im.shape[0], im.shape[1]) if u8 else (im.shape[1], im.shape[2]) for im in images]
    T = net.cfg.image_size
    o = default_overlap(T) if overlap is None else int(overlap)
    if tile_batch < 1:
        raise ValueError("tile_batch must be >= 1")
    odt = torch.float16 if net.output_f16 and not self_ensemble else torch.float32
    dev = images[0].device
    results = []
    keep_u8 = net.output_u8
    net.output_u8 = False              # the blend works on the float outputs; bytes come out of the blend, never get blended
    try:
        for first, last in pack_groups(sizes, T, o, int(tile_batch), 2 if odt == torch.float16 else 4, max_arena_bytes):
            plan = pack_plan(sizes[first:last], T, o, int(tile_batch))
            B = plan.B
            slab = 7 * B * T * T
            arena = torch.empty(plan.nslabs * slab, dtype=odt, device=dev)
            slab_in = torch.empty((B, T, T, 3) if u8 else (B, 3, T, T), dtype=images[0].dtype, device=dev)
            for s, segments in enumerate(plan.slabs):
                for k, t0, count, lane in segments:
                    _, ny, nx = plan.images[k]
                    ops.tile_gather(images[first + k], T, ny, nx, t0, count, out=slab_in[lane:lane + count])
                if self_ensemble:
                    ensemble.dehaze_x8(net, slab_in, out=arena[s * slab:(s + 1) * slab])
                else:
                    net(slab_in, out=arena[s * slab:(s + 1) * slab])
            for k, (slot0, ny, nx) in enumerate(plan.images):
                H, W = sizes[first + k]
                results.append(ops.tile_blend(arena[(slot0 // B) * slab:], B, T, H, W, ny, nx, o, output_u8=output_u8, lane0=slot0 % B))
    finally:
        net.output_u8 = keep_u8
    return results


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
