"""The integer resampling tables (cfen_vit_dehazing_amd/resample.py), applied in numpy (resample_ref.py), against Image.resize of the PIL
installed here, byte for byte; the table invariants the device pass relies on; the --fit refusals; the ledger of include/cfen_resample.h.
No GPU."""
import ctypes
import functools

import numpy as np
import pytest
from PIL import Image

from cfen_vit_dehazing_amd import resample
import cabi_ledger
import resample_ref as ref

SIZES = [(1, 1), (2, 3), (7, 5), (16, 16), (31, 47), (64, 64), (100, 37), (129, 255), (460, 620)]
# cost cap of the sweep: a pair runs when source + target pixels stay under it, which leaves out only the three pairs among the two largest sizes
# for the three optional filters; the two required filters run every pair
COST_CAP = 460 * 620 + 64 * 64


def _pairs(filter):
    for a in SIZES:
        for b in SIZES:
            if filter in ("bicubic", "bilinear") or a[0] * a[1] + b[0] * b[1] <= COST_CAP:
                yield a, b


def _images(shape, seed):
    rs = np.random.RandomState(seed)
    yield "random", rs.randint(0, 256, shape + (3,), dtype=np.uint8)
    yield "0/255", (rs.randint(0, 2, shape + (3,)) * 255).astype(np.uint8)        # drives the clip on both sides


@pytest.mark.parametrize("filter", resample.FILTERS)
def test_tables_applied_in_numpy_equal_pil_bitwise(filter):
    assert set(resample.FILTERS) >= {"bicubic", "bilinear"}
    n = 0
    for k, (a, b) in enumerate(_pairs(filter)):
        for kind, img in _images(a, k):
            want = ref.pil_resize(img, b, filter)
            got = ref.resize(img, b, filter)
            assert got.shape == want.shape and np.array_equal(got, want), (filter, a, b, kind)
            n += 1
    assert n >= 2 * (len(SIZES) ** 2 - 3)


@pytest.mark.parametrize("filter", resample.FILTERS)
def test_540x960_and_128x128_both_ways(filter):
    for a, b in (((540, 960), (128, 128)), ((128, 128), (540, 960))):
        for kind, img in _images(a, 5):
            assert np.array_equal(ref.resize(img, b, filter), ref.pil_resize(img, b, filter)), (filter, a, b, kind)


@pytest.mark.parametrize("filter", ["bicubic", "bilinear"])
def test_one_axis_only_and_equal_size(filter):
    img = next(_images((50, 64), 3))[1]
    for size in ((50, 32), (32, 64), (50, 100), (77, 64), (50, 64)):
        got = ref.resize(img, size, filter)
        assert np.array_equal(got, ref.pil_resize(img, size, filter)), size
    same = ref.resize(img, (50, 64), filter)
    assert same is not img and np.array_equal(same, img)                         # neither pass runs: a copy


@pytest.mark.parametrize("filter", resample.FILTERS)
def test_table_invariants(filter):
    edges = [1, 2, 3, 5, 7, 16, 31, 37, 47, 64, 100, 128, 129, 255, 460, 512, 540, 620, 960, 2160, 3840]
    for i in edges:
        for o in (1, 2, 5, 16, 17, 128, 512, 620, 3840):
            bounds, coef = resample.coefficients(i, o, filter)
            assert bounds.dtype == np.int32 and coef.dtype == np.int32 and bounds.shape == (o, 2) and coef.shape[0] == o
            xmin, n = bounds[:, 0].astype(np.int64), bounds[:, 1].astype(np.int64)
            assert (xmin >= 0).all() and (n >= 1).all() and (xmin + n <= i).all() and (n <= coef.shape[1]).all(), (i, o)
            assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + n) >= 0).all(), (i, o)          # the horizontal kernel stages [xmin_first, end_last)
            assert not coef[np.arange(coef.shape[1])[None, :] >= n[:, None]].any(), (i, o)        # zero padding
            assert 255 * int(np.abs(coef.astype(np.int64)).sum(axis=1).max()) + (1 << 21) < 1 << 31, (i, o)
            assert abs(int(coef.astype(np.int64).sum(axis=1).max()) - (1 << 22)) <= coef.shape[1], (i, o)
    assert resample.coefficients(960, 16, "bicubic")[1].shape[1] == 241 and resample.coefficients(540, 16, "bicubic")[1].shape[1] == 137
    assert resample.coefficients(3840, 512, "bicubic")[1].shape[1] == 31 and resample.coefficients(512, 3840, "bicubic")[1].shape[1] == 5
    assert resample.coefficients(64, 32, "bicubic")[0] is resample.coefficients(64, 32, "bicubic")[0]        # cached
    with pytest.raises(ValueError, match="unknown resampling filter"):
        resample.coefficients(4, 4, "nearest")
    with pytest.raises(ValueError):
        resample.coefficients(0, 4)


# ---- --fit at option parsing ----------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, *extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--name", "fit", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_fit_flags_and_refusals(tmp_path):
    opt = _parse(tmp_path)
    assert opt.fit is False and opt.fit_filter == "bicubic"
    opt = _parse(tmp_path, "--fit", "--fit_filter", "bilinear", "--batchSize", "4", "--resize_or_crop", "none")
    assert opt.fit is True and opt.fit_filter == "bilinear"
    for extra, names in ((["--fit", "--tile"], ("--fit", "--tile")), (["--fit", "--in_flight", "2"], ("--fit", "--in_flight")),
                         (["--fit", "--resize_or_crop", "resize_only"], ("--fit", "--resize_or_crop")),
                         (["--fit", "--resize_or_crop", "scale_width"], ("--fit", "--resize_or_crop"))):
        with pytest.raises(ValueError) as e:
            _parse(tmp_path, *extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    with pytest.raises(SystemExit):
        _parse(tmp_path, "--fit", "--fit_filter", "nearest")


def test_fit_hands_over_the_decoded_image(tmp_path):
    """with --fit the loader returns the (H,W,3) uint8 image whether --u8_input is given or not: the resample works on the bytes"""
    import torch
    from cfen_vit_dehazing_amd.data import get_transform
    img = Image.fromarray(np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3))
    for extra in ((), ("--u8_input",)):
        t = get_transform(_parse(tmp_path, "--fit", *extra))(img)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (5, 7, 3)
    assert get_transform(_parse(tmp_path))(img).dtype == torch.float32


# ---- the new header's ledger ----------------------------------------------------------------------------------------------------------------
def test_resample_header_is_exported_bound_and_apart_from_the_frozen_abi():
    cabi_ledger.check_header_bound("cfen_resample.h", {"cfen_resample_u8": 15})


def test_resample_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    src, tmp, dst, p, z = (ctypes.c_void_p(v) for v in (4096, 8192, 12288, 16384, 0))        # never dereferenced: every call is refused before a launch
    refused = functools.partial(cabi_ledger.refused, lib, "resample_u8")

    refused(b"null image pointer", z, 1, 4, 4, p, p, 5, 8, p, p, 5, 8, tmp, dst, z)
    refused(b"batch", src, 0, 4, 4, p, p, 5, 8, p, p, 5, 8, tmp, dst, z)
    refused(b"no horizontal table", src, 1, 4, 4, z, z, 0, 8, p, p, 5, 8, tmp, dst, z)
    refused(b"no vertical table", src, 1, 4, 4, p, p, 5, 8, z, z, 0, 8, tmp, dst, z)
    refused(b"horizontal table needs", src, 1, 4, 4, p, z, 5, 8, p, p, 5, 8, tmp, dst, z)
    refused(b"vertical table needs", src, 1, 4, 4, p, p, 5, 8, p, p, 0, 8, tmp, dst, z)
    refused(b"tmp", src, 1, 4, 4, p, p, 5, 8, p, p, 5, 8, z, dst, z)
    refused(b"different buffers", src, 1, 4, 4, p, p, 5, 8, p, p, 5, 8, tmp, src, z)
    refused(b"outside 1 ..", src, 1, 4, 1 << 20, p, p, 5, 8, p, p, 5, 8, tmp, dst, z)
