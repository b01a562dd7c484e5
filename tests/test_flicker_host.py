"""Flicker along the motion (include/cfen_flicker.h) on the host: the numpy restatement tests/flicker_ref.py against a plain loop over pixels, the
measure on the synthetic clips of DESIGN sections 18 and 20 (where the true camera path is known), cuts, batching, flicker.check_params, the
--eval_flicker options of dehaze_video.py, the csv and summary formats, the header's ledger and the argument errors of the two entry points.
No GPU."""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest

import cabi_ledger
import flicker_ref as ref
import motion_ref
import temporal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fkind", ref.FIELD_KINDS)
@pytest.mark.parametrize("kind,h,w,block,tol", [("random", 11, 13, 8, 255), ("shift", 9, 19, 8, 8), ("flat", 5, 7, 16, 0), ("shift", 17, 33, 16, 2)])
def test_the_vectorised_sums_are_the_plain_loop(kind, h, w, block, tol, fkind):
    f = motion_ref.frames(kind, h, w, 1, 5)
    t = motion_ref.frames("random", h, w, 1, 6)
    vec = ref.field(fkind, f[1:], f[0], block, 7)
    vec = None if vec is None else vec[0]
    got = ref.sums_one(f[1], f[0], t[1], t[0], vec, block, tol)
    want = ref.sums_plain(f[1], f[0], t[1], t[0], vec, block, tol)
    assert got.dtype == np.int64 and got.shape == (8,) and np.array_equal(got, want), (got, want)
    assert got[7] == 0 and got[1] <= got[0] <= h * w and got[2] <= got[6] and got[3] <= got[5]
    if fkind == "extreme":
        assert not got.any() and all(math.isnan(v) for v in ref.scores(got, h, w)[:3]) and ref.scores(got, h, w)[3:] == (0.0, 0.0)
    if fkind == "null":
        assert got[0] == h * w
    # scoring the input against itself: dF is dI
    own = ref.sums_one(f[1], f[0], f[1], f[0], vec, block, tol)
    assert own[2] == own[3] and own[5] == own[6]


def test_the_product_forms_the_scores_as_the_restatement_does():
    from cfen_vit_dehazing_amd import flicker
    assert flicker.CUT_SHARE == ref.CUT_SHARE == 0.5 and flicker.ROW_FIELDS == ref.FIELDS
    assert flicker.DEFAULTS == dict(range=8, block=16, bias=4, tol=8, down="auto")
    rs = np.random.RandomState(0)
    for n_match in (0, 7, 400):
        a = np.array([500, n_match, 3000, 9000, 123456, 9100, 3100, 0], np.int64)
        b = np.array([500, n_match, 3000, 4000, 23456, 4100, 3100, 0], np.int64)
        vec = rs.randint(-4, 5, (2, 3, 2)).astype(np.int16)
        want = ref.row(a, b, vec, 16, 25, 40)
        got = flicker.row_from_sums(a, b, int(np.abs(vec.astype(np.int64)).sum()), 6, 25, 40)
        assert set(got) == set(want)
        for k in want:
            assert got[k] == want[k] or (math.isnan(got[k]) and math.isnan(want[k])), (k, got[k], want[k])
        s = flicker.scores_from_sums(a, 25, 40)
        assert [s[k] for k in ("flicker", "hazy", "ewarp", "covered", "matched")] == pytest.approx(list(ref.scores(a, 25, 40)), abs=0, nan_ok=True)
    assert want["cut"] == 1 and ref.row(a, b, None, 16, 25, 20)["cut"] == 0 and ref.row(a, b, None, 16, 25, 20)["motion"] == 0.0


# ---- the measure on clips whose true camera path is known ------------------------------------------------------------------------------------------
def test_the_static_clip_is_the_plain_flicker():
    """a camera that does not move, the zero field, every pixel admitted: the pooled score of the network's frames over
    the frames 4 onward IS temporal_ref.flicker, bit for bit"""
    G, Y, _, _ = temporal_ref.jitter_stream(96, 128, 12, 3, 6.0, 0.04)
    rows = ref.Scorer(range=0, tol=255, down=1).step(G, Y)
    assert len(rows) == 11 and all(r["covered"] == 1.0 and r["matched"] == 1.0 and r["motion"] == 0.0 and not r["cut"] for r in rows)
    assert ref.pooled(rows[3:]) == temporal_ref.flicker(Y, 4) == 8.300262451171875


def _panning_rows(G, targets, R, tol):
    return [ref.Scorer(range=R, block=16, bias=4, tol=tol, down=1).step(G, F)[3:] for F in targets]


PANNING = (8.186, 8.184, 1.403)          # test_motion_host.PANNING: flicker_along_motion with the true origin
HARD = (8.268, 7.422, 4.432)             # the restatement's own values on the hard clip, searched field, tol 8
HARD_TRUE = (8.276, 7.420, 4.407)        # test_motion_host.HARD: the same clip along the true origin


@pytest.mark.parametrize("R,tol", [(4, 255), (4, 8), (8, 8)])
def test_the_clean_panning_clip_along_the_searched_field(R, tol):
    """DESIGN section 20's clip: the searched field (block 16, bias 4) scores what flicker_along_motion scores with the true origin"""
    G, Y, J, origin, alone, mc = motion_ref.panning_case(16, 4)
    rows = _panning_rows(G, (Y, alone, mc, J), R, tol)
    got = [ref.pooled(r) for r in rows]
    true = [motion_ref.flicker_along_motion(f, origin) for f in (Y, alone, mc)]
    print("R %d tol %d: pooled %s, along the true origin %s" % (R, tol, ["%.4f" % v for v in got], ["%.4f" % v for v in true]))
    assert np.allclose(got[:3], PANNING, atol=1e-3) and np.allclose(got[:3], true, atol=1e-3)
    assert got[3] == 0.0                                                                    # the clean frames do not flicker
    assert all(abs(r["covered"] - 0.966) < 1e-3 and r["matched"] == r["covered"] and r["hazy"] == 0.0 and not r["cut"] for r in rows[0])
    assert all(r["motion"] == 4.0 for r in rows[0])                                         # |1| + |3| in every block


def test_the_hard_panning_clip():
    """the same pan over a scene whose upper 40 % is a textureless sky, with sensor noise of 2 levels: the searched field is not the true one
    everywhere.  The restatement's values are pinned; the order holds; each lies within 2 % of its figure along the true origin"""
    G, Y, J, origin, alone, mc = motion_ref.panning_case(16, 4, sky=0.4, noise=2.0)
    rows = _panning_rows(G, (Y, alone, mc), 4, 8)
    net, al, co = (ref.pooled(r) for r in rows)
    hazy = ref.pooled(rows[0], "sad_hazy")
    matched = sum(r["n_matched"] for r in rows[0]) / sum(r["pixels"] for r in rows[0])
    print("pooled %.4f %.4f %.4f, hazy floor %.4f, matched %.4f" % (net, al, co, hazy, matched))
    assert np.allclose((net, al, co), HARD, atol=1e-3) and abs(hazy - 2.321) < 1e-3 and abs(matched - 0.974) < 1e-3
    assert co < al < net
    true = [motion_ref.flicker_along_motion(f, origin) for f in (Y, alone, mc)]
    assert np.allclose(true, HARD_TRUE, atol=1e-3)
    for got, want in zip((net, al, co), true):
        assert abs(got - want) <= 0.02 * want
    assert [r["n_matched"] for r in rows[0]] == [r["n_matched"] for r in rows[2]]           # every target is scored over the same pixels


def test_a_cut_is_marked_and_left_out():
    G, Y, _, _ = temporal_ref.jitter_stream(96, 128, 12, 3, 6.0, 0.04, moving=True, cut_at=6)
    rows = ref.Scorer(range=4, block=16, bias=4, tol=8, down=1).step(G, Y)
    assert len(rows) == 11
    print(["%.3f" % r["matched"] for r in rows])
    assert [r["cut"] for r in rows] == [0] * 5 + [1] + [0] * 5                              # row 5 is the pair (5, 6)
    assert rows[5]["matched"] < 0.05 and all(r["matched"] >= 0.96 for k, r in enumerate(rows) if k != 5)
    rest = rows[:5] + rows[6:]
    assert ref.pooled(rows) == ref.pooled(rest) == sum(r["sad_net"] for r in rest) / (3 * sum(r["n_matched"] for r in rest))
    from cfen_vit_dehazing_amd import flicker
    p = flicker.pool(rows)
    assert (p["pairs"], p["cuts"]) == (11, 1) and p["net"] == ref.pooled(rows) and p["hazy"] == ref.pooled(rows, "sad_hazy")
    assert p["ewarp_net"] == ref.pooled(rows, "sq_net", 255.0 ** 2) and p["out"] == p["net"]
    assert p["matched"] == sum(r["n_matched"] for r in rest) / (10 * 96 * 128)


def test_the_restatement_does_not_depend_on_batching():
    f = motion_ref.frames("shift", 26, 37, 11, 3)
    t = motion_ref.frames("random", 26, 37, 11, 4)
    o = motion_ref.frames("random", 26, 37, 11, 5)
    for down in (1, 2):
        kw = dict(range=3, block=8, bias=4, tol=8, down=down)
        want = ref.Scorer(**kw).step(f, t, o)
        assert len(want) == 11 and any(r["motion"] > 0 for r in want)
        for sizes in ((1,) * 12, (5, 7)):
            st, got, lo = ref.Scorer(**kw), [], 0
            for m in sizes:
                got += st.step(f[lo:lo + m], t[lo:lo + m], o[lo:lo + m])
                lo += m
            assert got == want, sizes


# ---- parameters and flags ----------------------------------------------------------------------------------------------------------------------------
def test_check_params():
    from cfen_vit_dehazing_amd import flicker
    assert flicker.check_params(8, 16, 4, 8, "auto") == (8, 16, 4, 8, "auto")
    assert flicker.check_params(np.int64(0), np.int32(32), 255.0, 0, 3) == (0, 32, 255, 0, 3)
    for bad, name in (((-1, 16, 4, 8, 1), "range"), ((17, 16, 4, 8, 1), "range"), ((2.5, 16, 4, 8, 1), "range"), ((None, 16, 4, 8, 1), "range"),
                      ((4, 12, 4, 8, 1), "block"), ((4, "16", 4, 8, 1), "block"), ((4, 16, -1, 8, 1), "bias"), ((4, 16, 256, 8, 1), "bias"),
                      ((4, 16, 4, -1, 1), "tol"), ((4, 16, 4, 256, 1), "tol"), ((4, 16, 4, 0.5, 1), "tol"), ((4, 16, 4, 8, 0), "down"),
                      ((4, 16, 4, 8, "2"), "down"), ((4, 16, 4, 8, 1.5), "down")):
        with pytest.raises(ValueError, match="Scorer: %s must be" % name):
            flicker.Scorer(*bad)
    st = flicker.Scorer()
    assert (st.range, st.block, st.bias, st.tol, st.down) == (8, 16, 4, 8, "auto")


def _parse(tmp_path, *extra, out=None):
    from cfen_vit_dehazing_amd.options.video_options import VideoOptions
    return VideoOptions().parse(["--in", "clip.y4m", "--out", out or str(tmp_path / "out.y4m"), "--name", "video", "--gpu_ids", "-1",
                                 "--checkpoints_dir", str(tmp_path / "ckpt")] + list(extra))


def test_eval_flicker_flags_and_refusals(tmp_path, capsys):
    for args in ((), ("--temporal",), ("--eval_noref",)):
        opt = _parse(tmp_path, *args)
        text = capsys.readouterr().out
        recorded = open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
        for t in (text, recorded):                                                          # a run without the flag prints and records what it always did
            assert not any(l.startswith(("eval_flicker", "flicker_")) for l in t.splitlines())
            assert "video_matrix: auto" in t and ("eval_noref: True" in t) == (args == ("--eval_noref",))
        assert not opt.eval_flicker
    opt = _parse(tmp_path, "--eval_flicker")
    assert (opt.flicker_range, opt.flicker_block, opt.flicker_bias, opt.flicker_tol, opt.flicker_down) == (8, 16, 4, 8, "auto")
    assert opt.flicker_csv == str(tmp_path / "flicker.csv")
    text = capsys.readouterr().out
    recorded = open(tmp_path / "ckpt" / "video" / "video_opt.txt").read()
    for t in (text, recorded):
        assert all(l in t for l in ("eval_flicker: True", "flicker_range: 8", "flicker_block: 16", "flicker_bias: 4", "flicker_tol: 8", "flicker_down: auto"))
    opt = _parse(tmp_path, "--eval_flicker", "--flicker_range", "0", "--flicker_block", "32", "--flicker_bias", "255", "--flicker_tol", "0",
                 "--flicker_down", "3", "--flicker_csv", str(tmp_path / "f.csv"), "--temporal", "--temporal_mc", "4", "--fit", "--eval_noref")
    assert (opt.flicker_range, opt.flicker_block, opt.flicker_bias, opt.flicker_tol, opt.flicker_down) == (0, 32, 255, 0, 3)
    assert opt.flicker_csv == str(tmp_path / "f.csv") and opt.temporal_mc == 4
    capsys.readouterr()
    for flag, value in (("--flicker_range", "4"), ("--flicker_block", "8"), ("--flicker_bias", "2"), ("--flicker_tol", "3"), ("--flicker_down", "2"),
                        ("--flicker_csv", "f.csv")):
        with pytest.raises(ValueError) as e:                                                # each needs --eval_flicker
            _parse(tmp_path, flag, value)
        assert flag in str(e.value) and "--eval_flicker" in str(e.value), str(e.value)
    for flag, values in (("--flicker_range", ("-1", "17")), ("--flicker_bias", ("-1", "256")), ("--flicker_tol", ("-1", "256")),
                         ("--flicker_down", ("0", "-2", "x", "1.5"))):
        for v in values:
            with pytest.raises(ValueError) as e:
                _parse(tmp_path, "--eval_flicker", "%s=%s" % (flag, v))
            assert flag + " must be" in str(e.value), (flag, v, str(e.value))
    for extra in (("--flicker_block", "12"), ("--flicker_range", "2.5"), ("--flicker_bias", "x"), ("--flicker_tol", "1e1")):
        with pytest.raises(SystemExit) as e:                                                # what argparse itself refuses leaves with 2 as well
            _parse(tmp_path, "--eval_flicker", *extra)
        assert e.value.code == 2
        assert extra[0] in capsys.readouterr().err
    with pytest.raises(ValueError, match="--flicker_csv PATH"):
        _parse(tmp_path, "--eval_flicker", out="-")
    assert _parse(tmp_path, "--eval_flicker", "--flicker_csv", "x.csv", out="-").flicker_csv == "x.csv"


def test_test_py_does_not_get_the_flag(capsys):
    """a folder of images is not a sequence"""
    from cfen_vit_dehazing_amd.options.test_options import TestOptions
    o = TestOptions()
    o.initialize()
    assert "flicker" not in o.parser.format_help()


# ---- the csv and the summary line --------------------------------------------------------------------------------------------------------------------
def test_csv_and_summary_formats():
    from cfen_vit_dehazing_amd import flicker
    assert flicker.CSV_HEADER == ("frame,motion,covered,matched,cut,hazy,net,out,ewarp_net,ewarp_out,pixels,n_matched,sad_hazy,sad_net,sad_out,"
                                  "sq_net,sq_out")
    a = np.array([1000, 800, 2400, 12000, 90000, 15000, 3100, 0], np.int64)
    b = np.array([1000, 800, 2400, 2400, 9000, 3000, 3100, 0], np.int64)
    z = np.array([1000, 0, 0, 0, 0, 15000, 99100, 0], np.int64)
    rows = [flicker.row_from_sums(a, b, 24, 6, 25, 40), flicker.row_from_sums(z, z, 0, 6, 25, 40), flicker.row_from_sums(a, a, 3, 6, 25, 40)]
    text = flicker.format_csv([("frame_%06d" % (k + 1), r) for k, r in enumerate(rows)])
    assert text == (flicker.CSV_HEADER + "\n"
                    "frame_000001,4.000000,1.000000,0.800000,0,1.000000,5.000000,1.000000,0.000577,0.000058,1000,800,2400,12000,2400,90000,9000\n"
                    "frame_000002,0.000000,1.000000,0.000000,1,nan,nan,nan,nan,nan,1000,0,0,0,0,0,0\n"
                    "frame_000003,0.500000,1.000000,0.800000,0,1.000000,5.000000,5.000000,0.000577,0.000577,1000,800,2400,12000,12000,90000,90000\n")
    assert flicker.summary_line(rows) == ("flicker: 3 frame pairs (1 cuts left out), matched 80.0 %, hazy 1.000, network 5.000 -> out 3.000 levels along "
                                          "the motion (B/A = 0.600), E_warp 0.000577 -> 0.000317")
    assert flicker.summary_line(rows[1:2]) == ("flicker: 1 frame pairs (1 cuts left out), matched nan %, hazy nan, network nan -> out nan levels along "
                                               "the motion (B/A = nan), E_warp nan -> nan")
    assert flicker.summary_line([]).startswith("flicker: 0 frame pairs (0 cuts left out), matched nan %")
    assert flicker.format_csv([]) == flicker.CSV_HEADER + "\n"


# ---- the new header's ledger -------------------------------------------------------------------------------------------------------------------------
def test_flicker_header_is_exported_bound_and_apart_from_the_older_tables():
    fns = {"cfen_flicker_bytes": 3, "cfen_flicker_u8": 13}
    cabi_ledger.check_header_bound("cfen_flicker.h", fns)
    cabi_ledger.check_guard_band_test_calls("test_hip_flicker.py", "test_guard_bands_flicker", fns)


def test_the_definition_stands_in_the_header():
    text = " ".join(re.sub(r"\n \*", "\n", open(os.path.join(ROOT, "include", "cfen_flicker.h")).read()).split())
    for phrase in ("q = p + v_b; it is NOT clamped", "covered(p) <=> q lies inside the frame", "dI(p) = sum_c |I_t(p, c) - I_{t-1}(q, c)|",
                   "dF(p) = sum_c |F_t(p, c) - F_{t-1}(q, c)|", "eF(p) = sum_c (F_t(p, c) - F_{t-1}(q, c))^2",
                   "matched(p) <=> covered(p) and dI(p) <= 3 * tol", "a NULL vec means all zeros", "Bk in {8, 16, 32}", "tol in 0 .. 255",
                   "0 n_cov 1 n_match 2 sum_matched dI 3 sum_matched dF 4 sum_matched eF 5 sum_covered dF 6 sum_covered dI 7 0 (reserved)",
                   "one call on n frames is bitwise n calls of one frame", "a source outside the frame is simply uncovered",
                   "flicker = sums[3] / (3 * sums[1])", "ewarp = sums[4] / (3 * sums[1] * 255^2)", "matched < 0.5 is a cut",
                   "4096 * 3 * 255^2 = 799 027 200 < 2^32", "The TILE is sized for the type"):
        assert phrase in text, phrase


# ---- the C entry points refuse bad arguments before any launch ---------------------------------------------------------------------------------------
def test_flicker_argument_errors_do_not_need_a_gpu():
    from cfen_vit_dehazing_amd import _lib
    lib = _lib.load()
    g, pg, t, pt, v, sc, su, z = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5, 6, 7, 0))      # never dereferenced
    refused, off = functools.partial(cabi_ledger.refused, lib, "flicker_u8"), cabi_ledger.off

    for i in (0, 1, 2, 3, 10, 11):
        args = [g, pg, t, pt, v, 1, 20, 20, 8, 8, sc, su, z]
        args[i] = z
        refused(b"null pointer", *args)
    refused(b"B = 0", g, pg, t, pt, v, 0, 20, 20, 8, 8, sc, su, z)
    refused(b"B = 65537", g, pg, t, pt, v, 65537, 20, 20, 8, 8, sc, su, z)
    refused(b"h = 0", g, pg, t, pt, v, 1, 0, 20, 8, 8, sc, su, z)
    refused(b"w = 16385", g, pg, t, pt, v, 1, 20, 16385, 8, 8, sc, su, z)
    for block in (0, 4, 12, 64, -8):
        refused(b"block = %d" % block, g, pg, t, pt, v, 1, 20, 20, block, 8, sc, su, z)
    refused(b"tol = -1", g, pg, t, pt, v, 1, 20, 20, 8, -1, sc, su, z)
    refused(b"tol = 256", g, pg, t, pt, v, 1, 20, 20, 8, 256, sc, su, z)
    for k in (1, 2, 3):
        refused(b"4-byte aligned", g, pg, t, pt, off(v, k), 1, 20, 20, 8, 8, sc, su, z)
    for bad in ((off(sc, 4), su), (sc, off(su, 4)), (off(sc, 1), su)):
        refused(b"8-byte aligned", g, pg, t, pt, v, 1, 20, 20, 8, 8, bad[0], bad[1], z)
    refused(b"too large for one launch", g, pg, t, pt, v, 65536, 16384, 16384, 8, 8, sc, su, z)
    # B = 2 frames of 20 x 20: guide and tgt 2400 bytes, the predecessors 1200, vec 2 * 9 * 4 = 72, scratch 2 * 32 = 64, sums 2 * 64 = 128
    for bad in ((g, su), (sc, sc), (sc, off(sc, 56)), (off(g, 2392), su), (sc, off(pg, 1192)), (off(t, -56), su), (sc, off(pt, -120)), (off(v, 64), su),
                (off(su, 120), su)):
        refused(b"must not overlap", g, pg, t, pt, v, 2, 20, 20, 8, 8, bad[0], bad[1], z)
    assert lib.cfen_flicker_bytes(2, 20, 20) == 64 and lib.cfen_flicker_bytes(3, 65, 129) == 3 * 2 * 3 * 32
    assert lib.cfen_flicker_bytes(65536, 16384, 64) == 65536 * 256 * 32
    for bad in ((0, 20, 20), (65537, 20, 20), (1, 0, 20), (1, 20, 0), (1, 16385, 20), (1, 20, 16385), (-1, 20, 20), (65536, 16384, 16384)):
        assert lib.cfen_flicker_bytes(*bad) == 0, bad
