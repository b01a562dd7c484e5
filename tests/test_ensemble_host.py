"""Self-ensemble (x8), the parts that need no GPU: the float64 restatement (ensemble_ref.py) against what the reference's Model.forward_x8 recorded
(tests/golden/ensemble_x8.npz, written by tools/gen_golden_ensemble.py), option parsing and refusals, C-ABI argument errors."""
import ctypes
import os

import numpy as np
import pytest

import ensemble_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ensemble_x8.npz")
# seven fp32 adds with partial sums of magnitude <= 8 (ulp 2^-21 in [4, 8): half an ulp each, 7 * 2^-22 at most, before the exact 1/8 -> 7 * 2^-25;
# the bar of the issue is the looser 7 * 2^-24
BAR = 7 * 2.0 ** -24


@pytest.fixture(scope="module")
def fixture():
    return np.load(GOLDEN)


def test_fixture_holds_the_cases(fixture):
    assert [str(n) for n in fixture["names"]] == list(ref.CASES)
    for name, (seed, C, T) in ref.CASES.items():
        assert fixture[name + "_x"].shape == (1, C, T, T) and fixture[name + "_x"].dtype == np.float32
        assert fixture[name + "_variants"].shape == (8, 1, C, T, T)
        assert fixture[name + "_ya"].shape == (8, 1, C, T, T) and fixture[name + "_yb"].shape == (8, 1, 1, T, T)
        assert fixture[name + "_out_a"].shape == (1, C, T, T) and fixture[name + "_out_b"].shape == (1, 1, T, T)


def test_restatement_reproduces_the_reference_variant_order_exactly(fixture):
    for name in ref.CASES:
        x = fixture[name + "_x"]
        got = ref.variants(x)
        assert np.array_equal(got, fixture[name + "_variants"]), name
        assert len({got[i].tobytes() for i in range(8)}) == 8, name                  # the eight really differ: the order is pinned, not vacuous


def test_recorded_forward_outputs_are_the_position_function_of_the_variants(fixture):
    for name, (seed, C, T) in ref.CASES.items():
        fn = ref.position_function(seed, C, T)
        for i in range(8):
            a, b = fn(fixture[name + "_variants"][i])
            assert np.array_equal(a, fixture[name + "_ya"][i]) and np.array_equal(b, fixture[name + "_yb"][i]), (name, i)
        # ... and that function is not equivariant: mapped back, the eight outputs differ
        z = [ref.back(fixture[name + "_ya"][i], i) for i in range(8)]
        assert all(np.abs(z[i] - z[0]).max() > 1e-2 for i in range(1, 8)), name


def test_restatement_outputs_are_within_the_bar_of_the_reference(fixture):
    assert 0 < float(fixture["max_ref32_f64"]) <= BAR
    worst = 0.0
    for name in ref.CASES:
        for k in ("a", "b"):
            want = fixture[name + "_out_" + k].astype(np.float64)
            got = ref.merge(fixture[name + "_y" + k])
            assert got.dtype == np.float64 and got.shape == want.shape
            worst = max(worst, float(np.abs(got - want).max()))
            assert np.abs(ref.merge_f32(fixture[name + "_y" + k]).astype(np.float64) - got).max() <= BAR
    print("max |reference fp32 - float64 restatement| = %.3e (bar %.3e)" % (worst, BAR))
    assert worst <= BAR
    assert abs(worst - float(fixture["max_ref32_f64"])) < 1e-12


def test_back_inverts_variant_and_the_transforms_are_the_variants():
    x = np.random.RandomState(0).uniform(-1, 1, (2, 3, 6, 6))
    for i in range(8):
        assert np.array_equal(ref.back(ref.variant(x, i), i), x)
        assert np.array_equal(ref.transform(x, i), ref.variant(x, i))
    assert np.array_equal(ref.variant(x, 1), x[..., ::-1]) and np.array_equal(ref.variant(x, 2), x[..., ::-1, :])
    assert np.array_equal(ref.variant(x, 4), np.swapaxes(x, -1, -2))
    assert np.array_equal(ref.variant(x, 7), np.swapaxes(x[..., ::-1, ::-1], -1, -2))          # v, then h, then t


# ---- options -------------------------------------------------------------------------------------------------------------------------------
def _parse(tmp_path, extra):
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    return TestOptions().parse(["--dataroot", str(tmp_path), "--checkpoints_dir", str(tmp_path / "ckpt"), "--gpu_ids", "-1"] + extra)


def test_flag_parses_and_is_refused_with_the_pipelined_driver(tmp_path, capsys):
    with pytest.raises(ValueError, match="--self_ensemble.*--in_flight 1"):
        _parse(tmp_path, ["--self_ensemble", "--in_flight", "2"])
    capsys.readouterr()
    opt = _parse(tmp_path, ["--self_ensemble", "--batchSize", "3", "--u8_input", "--precision", "half"])
    assert opt.self_ensemble is True
    assert "self_ensemble: True" in capsys.readouterr().out
    opt = _parse(tmp_path, ["--self_ensemble", "--tile", "--eval", "--sb", "--gpu_png", "--out_all"])
    assert opt.self_ensemble and opt.tile and opt.eval and opt.gpu_png
    capsys.readouterr()
    opt = _parse(tmp_path, ["--sb"])
    assert opt.self_ensemble is False
    keys = [line.split(":")[0] for line in capsys.readouterr().out.splitlines()]
    assert "tile" in keys and "self_ensemble" not in keys                 # a run without the flag prints the options it always printed


def test_python_entry_points_refuse_what_they_cannot_run():
    import torch
    from cfen_vit_dehazing_amd import ensemble, ops
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.hipnet import dec_ipt
    net = dec_ipt(NetConfig(24, 4, patch_size=8, load_size=64), compute_dtype="fp32")
    assert callable(net.forward_x8)
    with pytest.raises(ValueError, match="CUDA"):
        ensemble.dehaze_x8(net, torch.zeros(1, 3, 128, 128))              # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        ops.x8_expand(torch.zeros(1, 3, 128, 128))
    with pytest.raises(ValueError):
        ops.x8_merge(torch.zeros(56 * 16 * 16), 1, 16)
    import inspect
    from cfen_vit_dehazing_amd import tiled
    assert inspect.signature(tiled.dehaze_tiled).parameters["self_ensemble"].default is False


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_minus_one_without_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    P, N, S = ctypes.c_void_p(4096), ctypes.c_void_p(0), ctypes.c_void_p(0)
    ex = lambda u8, src, dst, M, m, T: lib.cfen_x8_expand(u8, src, dst, M, m, T, S)
    assert ex(0, N, P, 1, 0, 128) == -1 and b"null" in lib.cfen_last_error()
    assert ex(2, P, P, 1, 0, 128) == -1 and b"u8" in lib.cfen_last_error()
    assert ex(0, P, P, 1, 0, 120) == -1 and b"multiple of 16" in lib.cfen_last_error()
    assert ex(1, P, P, 1, 0, 0) == -1 and ex(1, P, P, 1, 0, 8) == -1 and ex(1, P, P, 1, 0, 16384) == -1
    assert ex(0, P, P, 2, 2, 128) == -1 and b"image 2" in lib.cfen_last_error()
    assert ex(0, P, P, 0, 0, 128) == -1 and ex(0, P, P, 1, -1, 128) == -1
    assert ex(0, ctypes.c_void_p(4100), P, 1, 0, 128) == -1 and b"aligned" in lib.cfen_last_error()
    assert ex(1, P, ctypes.c_void_p(4104), 1, 0, 128) == -1 and b"aligned" in lib.cfen_last_error()
    me = lambda dt, arena, M, T, u8, xr, xs, xd: lib.cfen_x8_merge(dt, arena, M, T, u8, xr, xs, xd, S)
    assert me(0, P, 1, 128, 0, P, P, N) == -1 and b"null" in lib.cfen_last_error()
    assert me(2, P, 1, 128, 0, P, P, P) == -1 and b"dtype" in lib.cfen_last_error()
    assert me(0, P, 1, 128, 2, P, P, P) == -1 and b"out_u8" in lib.cfen_last_error()
    assert me(1, P, 1, 136, 0, P, P, P) == -1 and b"multiple of 16" in lib.cfen_last_error()
    assert me(1, P, 0, 128, 0, P, P, P) == -1 and me(1, P, 5000, 128, 0, P, P, P) == -1 and b"images" in lib.cfen_last_error()
    assert me(0, ctypes.c_void_p(4104), 1, 128, 0, P, P, P) == -1 and b"aligned" in lib.cfen_last_error()
    assert me(0, P, 1, 128, 1, P, ctypes.c_void_p(4097), P) == -1 and b"aligned" in lib.cfen_last_error()
