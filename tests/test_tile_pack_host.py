"""Host side of packed tiled inference (tiled.pack_plan / pack_groups, the --tile_pack option): pure Python, no GPU."""
import pytest

from cfen_vit_dehazing_amd import tiled
from cfen_vit_dehazing_amd.options.test_options import TestOptions
import tiling_ref as ref

T, O = 128, 16
# tiles at T = 128, o = 16: 1, 2 x 3 = 6, 1 x 3 = 3, 1, 2 x 4 = 8 -> 19 tiles; with tile_batch 4: 5 slabs, 1 padded lane
GROUP = [(70, 45), (200, 300), (5, 300), (128, 128), (129, 383)]


def test_pack_plan_of_the_five_image_group():
    plan = tiled.pack_plan(GROUP, T, O, 4)
    assert plan.images == [(0, 1, 1), (1, 2, 3), (7, 1, 3), (10, 1, 1), (11, 2, 4)]
    assert [(ny, nx) for _, ny, nx in plan.images] == [(ref.n_tiles(H, T, O), ref.n_tiles(W, T, O)) for H, W in GROUP]
    assert plan.B == 4 and plan.nslabs == 5
    assert [slot0 % plan.B for slot0, _, _ in plan.images] == [0, 1, 3, 2, 3]          # the lane of every image's tile 0
    assert [slot0 // plan.B for slot0, _, _ in plan.images] == [0, 0, 1, 2, 2]
    assert plan.slabs == [[(0, 0, 1, 0), (1, 0, 3, 1)],
                          [(1, 3, 3, 0), (2, 0, 1, 3)],
                          [(2, 1, 2, 0), (3, 0, 1, 2), (4, 0, 1, 3)],
                          [(4, 1, 4, 0)],
                          [(4, 5, 4, 0)]]                                                 # 3 tiles left, the 4th lane is padding
    straddling = [k for k in range(len(GROUP)) if len({s for s, segs in enumerate(plan.slabs) for seg in segs if seg[0] == k}) > 1]
    assert straddling == [1, 2, 4]


@pytest.mark.parametrize("sizes,tile_batch", [(GROUP, 4), (GROUP, 8), (GROUP, 1), (GROUP, 19), (GROUP, 5), ([(460, 620)] * 3, 8), ([(128, 128)], 8),
                                              ([(300, 200), (1, 1)], 3)])
def test_every_lane_is_covered_once_and_only_the_last_segment_pads(sizes, tile_batch):
    plan = tiled.pack_plan(sizes, T, O, tile_batch)
    total = sum(ny * nx for _, ny, nx in plan.images)
    assert plan.B == min(tile_batch, total) and plan.nslabs == -(-total // plan.B) == len(plan.slabs)
    slot_of = {}                                              # global slot -> (image, tile) that the segments put there
    for s, segs in enumerate(plan.slabs):
        lanes = []
        for k, t0, count, lane in segs:
            n = plan.images[k][1] * plan.images[k][2]
            assert count >= 1 and 0 <= t0 < n and 0 <= lane and lane + count <= plan.B
            last = (s, (k, t0, count, lane)) == (plan.nslabs - 1, segs[-1])
            assert t0 + count <= n or last                    # only the very last segment runs past its image's tiles: the padding
            lanes += list(range(lane, lane + count))
            for b in range(count):
                slot_of[s * plan.B + lane + b] = (k, min(t0 + b, n - 1), t0 + b >= n)
        assert lanes == list(range(plan.B))                   # every lane of every slab exactly once, in order
    for k, (slot0, ny, nx) in enumerate(plan.images):
        for t in range(ny * nx):
            assert slot_of[slot0 + t] == (k, t, False)        # where the blend looks for tile t of image k: slot0 + t
    pad = [g for g, (_, _, padded) in slot_of.items() if padded]
    assert pad == list(range(total, plan.nslabs * plan.B))    # the padding is the tail of the last slab, copies of the last image's last tile
    assert all(slot_of[g][:2] == (len(sizes) - 1, plan.images[-1][1] * plan.images[-1][2] - 1) for g in pad)


def test_a_group_smaller_than_a_batch_runs_at_its_own_size():
    plan = tiled.pack_plan([(70, 45), (129, 300)], T, O, 8)
    assert plan.B == 7 and plan.nslabs == 1 and plan.slabs == [[(0, 0, 1, 0), (1, 0, 6, 1)]]
    one = tiled.pack_plan([(200, 300)], T, O, 4)              # one image: dehaze_tiled's own batches
    assert one.B == 4 and one.slabs == [[(0, 0, 4, 0)], [(0, 4, 4, 0)]]


def test_pack_plan_refuses_bad_arguments():
    with pytest.raises(ValueError):
        tiled.pack_plan([], T, O, 4)
    with pytest.raises(ValueError):
        tiled.pack_plan(GROUP, T, O, 0)
    with pytest.raises(ValueError):
        tiled.pack_plan([(0, 5)], T, O, 4)
    with pytest.raises(ValueError):
        tiled.pack_plan(GROUP, T, T, 4)


def test_groups_split_at_image_boundaries_under_a_small_arena_limit():
    slab4 = 7 * 4 * T * T * 4                                 # bytes of one fp32 slab of 4 tiles
    assert tiled.pack_groups(GROUP, T, O, 4, 4) == [(0, 5)]                               # the default limit holds them all
    assert tiled.pack_groups(GROUP, T, O, 4, 4, 5 * slab4) == [(0, 5)]
    # 2 slabs: images 0-1 are 7 tiles (2 slabs), + image 2 = 10 tiles (3 slabs) is over; 2-3 are 4 tiles (1 slab), + image 4 = 12 (3 slabs) is over
    groups = tiled.pack_groups(GROUP, T, O, 4, 4, 2 * slab4)
    assert groups == [(0, 2), (2, 4), (4, 5)]
    assert groups[0][0] == 0 and groups[-1][1] == len(GROUP) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
    for a, b in groups:
        plan = tiled.pack_plan(GROUP[a:b], T, O, 4)
        assert plan.nslabs * 7 * plan.B * T * T * 4 <= 2 * slab4
    assert tiled.pack_groups(GROUP, T, O, 4, 2, 2 * slab4) == [(0, 4), (4, 5)]            # fp16: 4 slabs fit -- 11 tiles do, 19 do not
    with pytest.raises(ValueError, match="a 200 x 300 image is 2 x 3 tiles"):             # one image alone (2 slabs) over the limit: dehaze_tiled's message
        tiled.pack_groups(GROUP, T, O, 4, 4, slab4)


def test_c_api_reads_lane0_from_the_dtype_argument_without_a_gpu():
    """every call fails an argument check before any launch (fake pointers never reach a kernel); WHICH check fails shows how dtype was read"""
    import ctypes
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    P, U, S = ctypes.c_void_p(4096), ctypes.c_void_p(4098), ctypes.c_void_p(0)

    def blend(dtype, B, xr=P):
        return lib.cfen_tile_blend(dtype, P, B, 128, 300, 200, 3, 2, 16, 0, xr, P, P, S), lib.cfen_last_error()

    for dtype in (0 | 8 << 8, 1 | 8 << 8, 0 | 0xffff << 8, 1 | 9 << 8):      # lane0 >= B = 8
        rc, msg = blend(dtype, 8)
        assert rc == -1 and b"lane0" in msg, msg
    for dtype in (1 << 24, 1 | 3 << 8 | 1 << 30, -1):                         # bits 24 and up
        rc, msg = blend(dtype, 8)
        assert rc == -1 and b"bits 24" in msg, msg
    for dtype in (2, 2 | 3 << 8, 0xff | 3 << 8):                              # the element type is bits 0..7 alone
        rc, msg = blend(dtype, 8)
        assert rc == -1 and b"unknown arena dtype" in msg, msg
    for dtype in (0, 1, 0 | 7 << 8, 1 | 7 << 8):                              # accepted: the call gets as far as the output alignment check
        rc, msg = blend(dtype, 8, xr=U)
        assert rc == -1 and b"aligned" in msg, msg


def _parse(tmp_path, extra):
    return TestOptions().parse(['--dataroot', str(tmp_path), '--name', 'x', '--gpu_ids', '-1', '--checkpoints_dir', str(tmp_path / 'ckpt')] + extra)


def test_tile_pack_option(tmp_path):
    assert _parse(tmp_path, []).tile_pack == 1
    assert _parse(tmp_path, ['--tile']).tile_pack == 1
    assert _parse(tmp_path, ['--tile', '--tile_pack', '1']).tile_pack == 1
    assert _parse(tmp_path, ['--tile_pack', '1']).tile_pack == 1                          # the default, spelled out, asks for nothing
    opt = _parse(tmp_path, ['--tile', '--tile_pack', '3', '--tile_batch', '4'])
    assert (opt.tile, opt.tile_pack, opt.tile_batch) == (True, 3, 4)
    with pytest.raises(ValueError, match="needs --tile"):
        _parse(tmp_path, ['--tile_pack', '2'])
    with pytest.raises(ValueError, match="--tile_pack"):
        _parse(tmp_path, ['--tile', '--tile_pack', '0'])
    with pytest.raises(ValueError, match="--in_flight"):
        _parse(tmp_path, ['--tile', '--tile_pack', '2', '--in_flight', '2'])
    with pytest.raises(ValueError):
        _parse(tmp_path, ['--tile_pack', '2', '--in_flight', '2'])
    with pytest.raises(ValueError, match="--batchSize 1"):                                # --tile keeps refusing batches of images
        _parse(tmp_path, ['--tile', '--batchSize', '2'])
    with pytest.raises(ValueError, match="--batchSize 1"):
        _parse(tmp_path, ['--tile', '--tile_pack', '2', '--batchSize', '2'])


def test_a_run_without_tile_pack_records_the_options_it_always_did(tmp_path):
    _parse(tmp_path, ['--tile'])
    assert not any(l.startswith('tile_pack') for l in open(tmp_path / 'ckpt' / 'x' / 'opt.txt'))
    _parse(tmp_path, ['--tile', '--tile_pack', '2'])
    assert 'tile_pack: 2\n' in list(open(tmp_path / 'ckpt' / 'x' / 'opt.txt'))
