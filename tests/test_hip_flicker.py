"""Flicker along the motion on the device (cfen_flicker_u8; ops.flicker_u8, flicker.Scorer, dehaze_video.py --eval_flicker).  The sums are
integers: they are held to the restatement tests/flicker_ref.py bit for bit, and so is everything built from them."""
import numpy as np
import pytest
import torch

from cfen_vit_dehazing_amd import _lib, flicker, ops, temporal
import flicker_ref as ref
import guarded
import motion_ref
import yuv_ref
from test_hip_temporal import CLIPS, _at_offset

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MANY_TILES = (70, 131)          # 2 x 3 tiles of 64 x 64 with partial tiles on both edges; 3 w is odd, so the rows start at every phase of a dword


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)          # a copy: the shared reference arrays are read-only


def same(t, a):
    return np.array_equal(t.cpu().numpy(), a)


def run(case, block, tol, **kw):
    guide, prev, tgt, prev_tgt, vec = (dev(a) for a in case[:5])
    return ops.flicker_u8(guide, prev, tgt, prev_tgt, vec, block, tol, **kw)


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------------------
def _check_every_kind(h, w, block, batches=(1, 3)):
    seen = set()
    for kind in ref.KINDS:
        for fkind in ref.FIELD_KINDS:
            for B in batches:
                case = ref.sums_case(kind, fkind, h, w, block, B)
                for tol in ref.TOLS:
                    got = run(case, block, tol)
                    assert got.shape == (B, 8) and got.dtype == torch.int64
                    assert same(got, case[5][tol]), (kind, fkind, B, tol, got.cpu().numpy(), case[5][tol])
                want = case[5][8]
                if fkind == "extreme":
                    assert not want.any()                        # nothing is covered: every score is nan
                    assert all(np.isnan(flicker.scores_from_sums(want[0], h, w)[k]) for k in ("flicker", "hazy", "ewarp"))
                seen |= {(fkind, bool(want[:, 0].any()), bool((want[:, 1] < want[:, 0]).any()))}
                # the input scored against itself, through the same pointers: dF is dI
                guide, prev, vec = dev(case[0]), dev(case[1]), dev(case[4])
                own = ops.flicker_u8(guide, prev, guide, prev, vec, block, 8).cpu().numpy()
                assert np.array_equal(own, ref.sums(case[0], case[1], case[0], case[1], case[4], block, 8))
                assert np.array_equal(own[:, 2], own[:, 3]) and np.array_equal(own[:, 5], own[:, 6])
    return seen


@pytest.mark.parametrize("block", ref.BLOCKS)
@pytest.mark.parametrize("h,w", ref.SIZES)
def test_sums_bitwise(h, w, block):
    """every kind of content and field, B = 1 and 3, tol 0, 8 and 255, and the target aliasing the guide"""
    seen = _check_every_kind(h, w, block)
    assert ("extreme", False, False) in seen and ("null", True, True) in seen          # nothing covered; all covered and some of it not matched


def test_sums_bitwise_over_several_tiles():
    h, w = MANY_TILES
    assert _lib.load().cfen_flicker_bytes(2, h, w) == 2 * 6 * 32
    _check_every_kind(h, w, 16, batches=(2,))
    _check_every_kind(h, w, 8, batches=(1,))


def test_no_partial_overflows():
    """all-255 against all-0 frames of 2400 x 2400: a tile's largest partial is 4096 * 195075, the frame's sums pass 2^32 (and so does the
    sum of the tiles' partials, which is why the second launch adds them in 64 bits)"""
    h = w = 2400
    N = h * w
    cur = torch.full((1, h, w, 3), 255, dtype=torch.uint8, device=DEV)
    prev = torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV)
    got = ops.flicker_u8(cur, prev, cur, prev, None, 16, 255).cpu().tolist()
    assert N == 5760000 and 195075 * N > 1 << 32 and 765 * N > 1 << 32
    assert got == [[N, N, 765 * N, 765 * N, 195075 * N, 765 * N, 765 * N, 0]]


def test_a_frame_alone_is_the_frame_in_a_batch_and_on_a_side_stream():
    h, w = MANY_TILES
    case = ref.sums_case("shift", "searched", h, w, 16, 3)
    guide, prev, tgt, prev_tgt, vec = (dev(a) for a in case[:5])
    want = case[5][8]
    got = ops.flicker_u8(guide, prev, tgt, prev_tgt, vec, 16, 8)
    assert same(got, want)
    for k in range(3):
        one = ops.flicker_u8(guide[k:k + 1], guide[k - 1] if k else prev, tgt[k:k + 1], tgt[k - 1] if k else prev_tgt, vec[k:k + 1], 16, 8)
        assert torch.equal(one[0], got[k]), k
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        there = ops.flicker_u8(guide, prev, tgt, prev_tgt, vec, 16, 8)
    side.synchronize()
    assert torch.equal(there, got)
    out = torch.empty(3, 8, dtype=torch.int64, device=DEV)
    assert ops.flicker_u8(guide, prev, tgt, prev_tgt, vec, 16, 8, out=out).data_ptr() == out.data_ptr() and torch.equal(out, got)


@pytest.mark.parametrize("h,w", [(17, 33), MANY_TILES])
def test_byte_offsets(h, w):
    """each of the four frame buffers 1 .. 3 bytes past a 16-byte boundary, alone and together: the dword and the byte path give the same sums"""
    case = ref.sums_case("shift", "random", h, w, 8, 3)
    vec, want = dev(case[4]), case[5][8]
    for k in (1, 2, 3):
        for ks in ((k, 0, 0, 0), (0, k, 0, 0), (0, 0, k, 0), (0, 0, 0, k), (k, k, k, k), (k, (k + 1) % 4, (k + 2) % 4, (k + 3) % 4)):
            bufs = [_at_offset(a, o) for a, o in zip(case[:4], ks)]
            assert same(ops.flicker_u8(bufs[0], bufs[1], bufs[2], bufs[3], vec, 8, 8), want), ks


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------------------
def test_guard_bands_flicker():
    """every input between 0xff bands, the scratch and the sums between random bands and prefilled with 0xff, zeros and random bytes: no band
    changes, and the sums are the restatement's whatever the two held before"""
    lib = _lib.load()
    for (h, w), block, fkind in (((17, 33), 8, "random"), (MANY_TILES, 32, "searched"), ((5, 7), 16, "null"), ((40, 50), 16, "extreme")):
        case = ref.sums_case("shift", fkind, h, w, block, 3)
        ins = [guarded.guarded_copy(dev(a)) for a in case[:4]]
        tv = guarded.guarded_copy(dev(case[4])) if case[4] is not None else None
        nbytes = lib.cfen_flicker_bytes(3, h, w)
        assert nbytes == 3 * (-(-h // 64)) * (-(-w // 64)) * 32
        scratch = guarded.guarded_empty((nbytes,), torch.uint8, DEV)
        sums = guarded.guarded_empty((3, 8), torch.int64, DEV)
        for fill in guarded.FILLS:
            guarded.refill(scratch, fill)
            guarded.refill(sums, fill)
            _lib.check(lib.cfen_flicker_u8(_lib.ptr(ins[0]), _lib.ptr(ins[1]), _lib.ptr(ins[2]), _lib.ptr(ins[3]), _lib.ptr(tv), 3, h, w, block, 8,
                                           _lib.ptr(scratch), _lib.ptr(sums), _lib.current_stream()), "flicker_u8")
            torch.cuda.synchronize()
            guarded.check_bands(scratch, sums, *ins, *([tv] if tv is not None else []))
            assert same(sums, case[5][8]), (h, w, fill)
            records = scratch.cpu().numpy().view(np.uint32).reshape(3, -1, 8)
            assert np.array_equal(records.astype(np.int64).sum(axis=1), case[5][8])          # every record was written: one per tile


def test_argument_errors_launch_nothing():
    h, w = 20, 20
    f = dev(motion_ref.frames("random", h, w, 2, 1))
    g, p = f[1:], f[0]                                           # B = 2
    vec = torch.zeros(2, 3, 3, 2, dtype=torch.int16, device=DEV)
    out = torch.full((2, 8), 7, dtype=torch.int64, device=DEV)
    for bad in ({"block": 12}, {"block": 8.5}, {"tol": -1}, {"tol": 256}, {"tol": 2.5}):
        with pytest.raises(ValueError, match="flicker_u8: (block|tol)"):
            ops.flicker_u8(g, p, g, p, None, **dict({"block": 8, "tol": 8}, **bad), out=out)
    with pytest.raises(ValueError, match="needs prev_guide"):
        ops.flicker_u8(g, p[:10], g, p, None, 8, 8, out=out)
    with pytest.raises(ValueError, match="needs prev_tgt"):
        ops.flicker_u8(g, p, g, p.float(), None, 8, 8, out=out)
    with pytest.raises(ValueError, match="differ in shape"):
        ops.flicker_u8(g, p, f, p, None, 8, 8, out=out)
    with pytest.raises(ValueError, match="needs vec"):
        ops.flicker_u8(g, p, g, p, vec[:1], 8, 8, out=out)
    with pytest.raises(ValueError, match="needs vec"):
        ops.flicker_u8(g, p, g, p, vec.int(), 8, 8, out=out)
    with pytest.raises(ValueError, match="out must be"):
        ops.flicker_u8(g, p, g, p, vec, 8, 8, out=out[:1])
    with pytest.raises(ValueError, match="out must be"):
        ops.flicker_u8(g, p, g, p, vec, 8, 8, out=out.int())
    lib = _lib.load()
    scratch = torch.full((16,), 7, dtype=torch.int64, device=DEV)

    def raw(sc, su):
        return lib.cfen_flicker_u8(_lib.ptr(g), _lib.ptr(p), _lib.ptr(g), _lib.ptr(p), _lib.ptr(vec), 2, h, w, 8, 8, _lib.ptr(sc), _lib.ptr(su),
                                   _lib.current_stream())

    # the outputs overlap each other, or an input (scratch: 2 records of 32 bytes; sums: 128 bytes)
    for sc, su in ((scratch, scratch), (scratch, scratch[4:]), (out.view(-1)[:8], out), (scratch, g.view(-1)[:128].view(torch.int64))):
        assert raw(sc, su) == -1 and b"must not overlap" in lib.cfen_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((scratch == 7).all()) and not bool(vec.any())
    assert raw(scratch, out) == 0                                # and the same call with the outputs apart runs
    torch.cuda.synchronize()
    assert same(out, ref.sums(g.cpu().numpy(), p.cpu().numpy(), g.cpu().numpy(), p.cpu().numpy(), None, 8, 8))


# ---- the Scorer -------------------------------------------------------------------------------------------------------------------------------------
def _compose(tG, tN, tO, R=4, block=16, bias=4, tol=8, down=1):
    """the Scorer written out with the operators, frame by frame: rows"""
    n, H, W, _ = tG.shape
    S, h, w = temporal.working_size(H, W, down)
    I, N, O = ((tG, tN, tO) if S == 1 else tuple(ops.resample_u8(t, (h, w), filter="box") for t in (tG, tN, tO)))
    rows = []
    nblocks = -(-h // block) * -(-w // block)
    for k in range(1, n):
        vec = ops.motion_search_u8(I[k:k + 1], I[k - 1], block, R, bias)[0] if R else None
        a = ops.flicker_u8(I[k:k + 1], I[k - 1], N[k:k + 1], N[k - 1], vec, block, tol)[0].cpu().tolist()
        b = ops.flicker_u8(I[k:k + 1], I[k - 1], O[k:k + 1], O[k - 1], vec, block, tol)[0].cpu().tolist()
        l1 = int(np.abs(vec.cpu().numpy().astype(np.int64)).sum()) if vec is not None else 0
        rows.append(flicker.row_from_sums(a, b, l1, nblocks, h, w))
    return rows


def _equal_rows(got, want):
    return len(got) == len(want) and all(g.keys() == w.keys() and all(g[k] == w[k] or (g[k] != g[k] and w[k] != w[k]) for k in w) for g, w in zip(got, want))


@pytest.mark.parametrize("H,W,down,block,R", [(40, 64, 1, 16, 4), (75, 101, 2, 8, 4), (45, 71, 1, 32, 0)])
def test_scorer_is_the_composition_of_its_operators_and_does_not_depend_on_batching(H, W, down, block, R):
    from test_hip_motion import _pan
    G, Y = _pan(5, H, W, H, step=(down, 3 * down))
    O = np.clip(Y.astype(np.int64) + np.random.RandomState(W).randint(-3, 4, (5, 1, 1, 3)), 0, 255).astype(np.uint8)
    tG, tY, tO = dev(G), dev(Y), dev(O)
    want = _compose(tG, tY, tO, R=R, block=block, down=down)
    assert len(want) == 4 and (all(r["motion"] > 0 for r in want) if R else not any(r["motion"] for r in want))
    host = ref.Scorer(range=R, block=block, bias=4, tol=8, down=down).step(G, Y, O)          # and the restatement's rows, bit for bit
    assert _equal_rows(want, host)
    for sizes in ((5,), (1, 1, 1, 1, 1), (2, 2, 1), (1, 4)):
        sc = flicker.Scorer(range=R, block=block, down=down)
        got, lo = [], 0
        for m in sizes:
            got += sc.step(tG[lo:lo + m], tY[lo:lo + m], tO[lo:lo + m])
            lo += m
        assert _equal_rows(got, want), sizes
    # without a second target, or with the network's own tensor as the second, the two columns are equal and one call is made
    sc = flicker.Scorer(range=R, block=block, down=down)
    alone = sc.step(tG[:3], tY[:3]) + sc.step(tG[3:], tY[3:], tY[3:])
    assert _equal_rows(alone, _compose(tG, tY, tY, R=R, block=block, down=down)) and all(r["net"] == r["out"] for r in alone)
    sc.reset()
    assert sc.step(tG[:1], tY[:1]) == [] and len(sc.step(tG[1:], tY[1:])) == 4
    with pytest.raises(ValueError, match="reset"):
        sc.step(tG[:, :20].contiguous(), tY[:, :20].contiguous())


def test_the_panning_clip_on_the_device():
    """the clip of DESIGN section 20: the pooled figures of the network's frames, of --temporal alone and of the compensated run (the
    restatement's frames) from the device's rows are the restatement's, and those are test_flicker_host's"""
    G, Y, J, origin, alone, mc = motion_ref.panning_case(16, 4)
    tG = dev(G)
    for frames, pinned in ((Y, 8.186), (alone, 8.184), (mc, 1.403)):
        got = flicker.Scorer(range=motion_ref.PAN_RANGE, down=1).step(tG, dev(frames))[3:]
        want = ref.Scorer(range=motion_ref.PAN_RANGE, down=1).step(G, frames)[3:]
        assert _equal_rows(got, want)
        assert flicker.pool(got)["net"] == ref.pooled(want) and abs(ref.pooled(want) - pinned) < 1e-3


# ---- dehaze_video.py --eval_flicker -----------------------------------------------------------------------------------------------------------------
CLI = {"plain": ("plain", []), "fit": ("fit", []), "temporal_mc": ("plain", ["--temporal", "--temporal_mc", "4"])}


@pytest.mark.parametrize("case", list(CLI))
def test_cli_eval_flicker(case, tmp_path):
    """dehaze_video.py --eval_flicker in child processes: flicker.csv is, byte for byte, library route -> (Stabiliser) -> the composition above;
    the same at --batchSize 1 and 2; the stream and noref.csv are what the run without the flag writes"""
    import test_hip_video as vid
    from test_hip_motion import _panned_stream
    route, extra = CLI[case]
    n, H, W, chroma, flags = CLIPS[route]
    vid._setup(tmp_path)
    data, header, rgb = _panned_stream(n, H, W, chroma)
    (tmp_path / "in.y4m").write_bytes(data)
    net = vid._net()
    x = dev(np.stack(rgb))
    with torch.no_grad():
        outs = []
        for lo in range(0, n, 2):
            if route == "plain":
                net.output_u8 = True
                outs.append(net(x[lo:lo + 2])[2])
                net.output_u8 = False
            else:
                outs.append(net.forward_fit(x[lo:lo + 2])[2])
    y = torch.cat(outs).contiguous()
    out = y
    if extra:
        st = temporal.Stabiliser(mc_range=4)
        out = torch.cat([st.step(x[lo:lo + 2], y[lo:lo + 2]) for lo in range(0, n, 2)])
        assert not torch.equal(out, y)
    d = flicker.DEFAULTS
    rows = _compose(x, y, out, R=d["range"], block=d["block"], bias=d["bias"], tol=d["tol"], down="auto")
    want = flicker.format_csv([("frame_%06d" % (k + 1), r) for k, r in enumerate(rows)])
    assert len(rows) == n - 1 and any(r["motion"] > 0 for r in rows) and (bool(extra) == any(r["net"] != r["out"] for r in rows))

    for bs in ("2", "1"):
        sub = tmp_path / ("with_%s" % bs)
        sub.mkdir()
        r = vid._run(tmp_path, tmp_path / "in.y4m", sub / "out.y4m", flags + extra + ["--batchSize", bs, "--eval_flicker"] + (["--eval_noref"] if bs == "2" else []))
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        text = r.stdout.decode()
        assert "eval_flicker: True" in text and "flicker_range: 8" in text and "video: flicker along the motion at %d x %d (1/1)" % (W, H) in text
        assert flicker.summary_line(rows) in text and "flicker: wrote %s" % (sub / "flicker.csv") in text
        assert (sub / "flicker.csv").read_text() == want, bs
    sub = tmp_path / "without"
    sub.mkdir()
    r = vid._run(tmp_path, tmp_path / "in.y4m", sub / "out.y4m", flags + extra + ["--batchSize", "2", "--eval_noref"])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "flicker" not in r.stdout.decode().replace(str(tmp_path), "") and not (sub / "flicker.csv").exists()
    assert (sub / "out.y4m").read_bytes() == (tmp_path / "with_2" / "out.y4m").read_bytes() == (tmp_path / "with_1" / "out.y4m").read_bytes()
    assert (sub / "noref.csv").read_bytes() == (tmp_path / "with_2" / "noref.csv").read_bytes()
    got_header, got = yuv_ref.y4m_frames((sub / "out.y4m").read_bytes(), H, W, chroma)
    assert got_header == header and all(np.array_equal(got[k], yuv_ref.rgb_to_yuv(out[k].cpu().numpy(), chroma, "bt601", False)) for k in range(n))
    if case == "plain":                                        # a refusal leaves with 2, names the flag and writes nothing
        r = vid._run(tmp_path, tmp_path / "in.y4m", tmp_path / "none.y4m", ["--eval_flicker", "--flicker_range", "17"])
        assert r.returncode == 2 and b"--flicker_range" in r.stderr and not (tmp_path / "none.y4m").exists()
