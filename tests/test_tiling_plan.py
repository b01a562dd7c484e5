"""Tile plan of overlapping-tile inference (tiled.tile_grid) against the definitions, and the float64 reference gather / blend the GPU tests
compare with (no GPU needed)."""
import numpy as np
import pytest

from cfen_vit_dehazing_amd import tiled
import tiling_ref as ref

SIZES = [1, 2, 45, 127, 128, 129, 300, 413, 460, 511, 512, 513, 550, 620, 1080, 1920, 2160, 3840]


@pytest.mark.parametrize("T", [128, 512])
@pytest.mark.parametrize("o_kind", ["zero", "small", "default", "half"])
def test_grid_covers_flush_monotone_and_overlaps(T, o_kind):
    o = {"zero": 0, "small": 16, "default": T // 8, "half": T // 2}[o_kind]
    for L in SIZES:
        ys, xs = tiled.tile_grid(L, 7, T, o)
        assert xs == [0]
        n = len(ys)
        assert n == ref.n_tiles(L, T, o) and ys == ref.origins(L, T, o)
        assert ys[0] == 0
        if L >= T:
            assert ys[-1] + T == L                              # flush with the far edge
        covered = np.zeros(L, dtype=bool)
        for p in ys:
            covered[p:p + T] = True
        assert covered.all()
        assert all(a < b for a, b in zip(ys, ys[1:]))          # monotone
        steps = [b - a for a, b in zip(ys, ys[1:])]
        if steps:
            assert max(steps) - min(steps) <= 1                 # evenly spread
            assert max(steps) <= T - o                          # neighbours overlap by >= o


@pytest.mark.parametrize("T,o", [(128, 16), (512, 64), (512, 0), (512, 256)])
def test_tile_count_formula(T, o):
    for L in (1, T - 1, T, T + 1, 2 * T - o, 3840):
        want = 1 if L <= T else 1 + -(-(L - T) // (T - o))
        assert tiled.tile_count(L, T, o) == want
        assert len(tiled.tile_grid(L, L, T, o)[0]) == want
    assert tiled.tile_count(2 * T - o, T, o) == 2
    assert tiled.tile_count(2 * T - o + 1, T, o) == 3


def test_4k_plan_is_9_by_5_at_512():
    ys, xs = tiled.tile_grid(2160, 3840, 512, tiled.default_overlap(512))
    assert (len(ys), len(xs)) == (5, 9)


@pytest.mark.parametrize("bad", [-1, 65, 1000])
def test_bad_overlap_raises(bad):
    with pytest.raises(ValueError):
        tiled.tile_grid(300, 300, 128, bad)


def test_bad_size_raises():
    for H, W, T, o in ((0, 5, 128, 16), (5, 0, 128, 16), (5, 5, 1, 0), (5.0, 5, 128, 16)):
        with pytest.raises(ValueError):
            tiled.tile_grid(H, W, T, o)


def test_mirror_is_numpy_reflect():
    for L in (1, 2, 3, 7, 45):
        k = np.arange(0, 300)
        want = np.pad(np.arange(L), (0, 300), mode="reflect")[:300] if L > 1 else np.zeros(300, dtype=int)
        assert np.array_equal(ref.mirror(k, L), want)


@pytest.mark.parametrize("H,W,T,o", [(300, 200, 128, 16), (70, 45, 128, 16), (460, 620, 128, 64), (129, 1, 128, 0), (1080, 1920, 512, 64)])
def test_reference_blend_of_constant_tiles_is_constant(H, W, T, o):
    n = ref.n_tiles(H, T, o) * ref.n_tiles(W, T, o)
    tiles = np.full((n, 7, T, T), 0.375)
    out, cnt = ref.blend(tiles, H, W, T, o)
    assert out.shape == (7, H, W) and (cnt >= 1).all()
    assert np.abs(out - 0.375).max() < 1e-12


def test_reference_single_tile_maps_onto_itself():
    rs = np.random.RandomState(0)
    T = 128
    img = rs.rand(T, T, 3)
    tiles = ref.gather(img, T, 16, hwc=True)
    assert tiles.shape == (1, T, T, 3) and np.array_equal(tiles[0], img)
    out, cnt = ref.blend(tiles.transpose(0, 3, 1, 2), T, T, T, 16)
    assert (cnt == 1).all() and np.array_equal(out, img.transpose(2, 0, 1))


def test_reference_gather_mirrors_small_images():
    img = np.arange(45 * 70 * 3).reshape(3, 70, 45).astype(np.float64)
    tiles = ref.gather(img, 128, 16, hwc=False)
    assert tiles.shape == (1, 3, 128, 128)
    want = np.pad(img, ((0, 0), (0, 128 - 70), (0, 128 - 45)), mode="reflect")
    assert np.array_equal(tiles[0], want)


def test_c_api_refuses_bad_plans_without_a_gpu():
    """every call below fails its argument checks before any launch (fake pointers never reach a kernel)"""
    import ctypes
    from cfen_vit_dehazing_amd import _lib
    if not hasattr(_lib.load(), "cfen_tile_blend"):
        pytest.fail("libcfen_hip.so predates cfen_tile_blend: rebuild")
    lib = _lib.load()
    P = ctypes.c_void_p(4096)
    S = ctypes.c_void_p(0)
    # blend: overlap > T/2, overlap < 0, a grid that is not the plan, empty image, unaligned output
    assert lib.cfen_tile_blend(0, P, 8, 128, 300, 200, 3, 2, 65, 0, P, P, P, S) == -1
    assert b"overlap" in lib.cfen_last_error()
    assert lib.cfen_tile_blend(0, P, 8, 128, 300, 200, 3, 2, -1, 0, P, P, P, S) == -1
    assert lib.cfen_tile_blend(0, P, 8, 128, 300, 200, 2, 2, 16, 0, P, P, P, S) == -1
    assert b"300 x 200" in lib.cfen_last_error()
    assert lib.cfen_tile_blend(0, P, 8, 128, 0, 200, 1, 2, 16, 0, P, P, P, S) == -1
    assert lib.cfen_tile_blend(0, P, 8, 128, 300, 200, 3, 2, 16, 0, ctypes.c_void_p(4098), P, P, S) == -1
    assert lib.cfen_tile_blend(2, P, 8, 128, 300, 200, 3, 2, 16, 0, P, P, P, S) == -1
    # gather: T not a multiple of 16, a grid that leaves pixels out, t0 past the tiles, unaligned slab
    assert lib.cfen_tile_gather(1, P, P, 300, 200, 120, 3, 2, 0, 8, S) == -1
    assert lib.cfen_tile_gather(1, P, P, 300, 200, 128, 2, 1, 0, 8, S) == -1
    assert lib.cfen_tile_gather(1, P, P, 300, 200, 128, 3, 2, 6, 8, S) == -1
    assert lib.cfen_tile_gather(0, P, ctypes.c_void_p(4100), 300, 200, 128, 3, 2, 0, 8, S) == -1
    assert lib.cfen_tile_gather(0, P, P, 100, 200, 128, 2, 2, 0, 8, S) == -1       # H <= T needs one tile row
