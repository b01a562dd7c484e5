"""dehaze_video.py --eval_gt in child processes: gt.csv is gtscore.format_csv of the restatement tests/planes_ref.py applied to (the stream the
run wrote, the ground-truth file) -- integers exact, SSIM within the bar of tests/test_hip_plane_metrics.py -- whatever the batch size, the
number of buffers and the route; the stream is byte for byte the one of the run without the flag; refusals leave with 2 before the checkpoint
is looked for.  The tiny seeded checkpoint and the streams are those of test_hip_video.py / test_hip_video_deep.py."""
import os

import numpy as np
import pytest

from cfen_vit_dehazing_amd import gtscore
import planes_ref as ref
import test_hip_video as vid
import test_hip_video_deep as deep
from test_hip_video_deep import ckpt          # noqa: F401  (the module-scoped checkpoint fixture: one file, linked where one exists)

pytestmark = pytest.mark.gpu

ROOT = deep.ROOT
SSIM_COLUMNS = (5, 6, 7)


def _golden_distance():
    return float(np.load(os.path.join(ROOT, "tests", "golden", "metrics_pairs.npz"))["max_ref32_f64"])


def _check_csv(text, out_bytes, gt_bytes, H, W, chroma, depth, what):
    """text: the gt.csv a run wrote; out_bytes, gt_bytes: the y4m files.  Every cell formed from integers is the restatement's text; an SSIM cell
    lies within 2 D (+ the cell's own rounding) of float64, D the fp32 distance of test_hip_plane_metrics.py: the golden file's at depth 8, at a
    deeper depth the distance of the fp32 numpy evaluation over this very pair of streams"""
    out, gt = ref.y4m_payloads(out_bytes, H, W, chroma, depth)[1], ref.y4m_payloads(gt_bytes, H, W, chroma, depth)[1]
    n = out.shape[0]
    assert gt.shape[0] >= n
    w = ref.words(out, gt[:n], H, W, chroma, depth)
    if depth == 8:
        dist = _golden_distance()
    else:
        dist = float(np.nanmax(np.abs(w[2] - ref.words(out, gt[:n], H, W, chroma, depth, dtype=np.float32)[2])))
        assert dist > 0.0
    rows = [gtscore.row_from_words(w[0][k], w[1][k], w[2][k], w[3][k], depth, k > 0) for k in range(n)]
    want = gtscore.format_csv([("frame_%06d" % k, r) for k, r in enumerate(rows)]).splitlines()
    got = text.splitlines()
    assert len(got) == len(want) == n + 1 and got[0] == want[0] == gtscore.CSV_HEADER and text.endswith("\n")
    worst = 0.0
    for g, x in zip(got[1:], want[1:]):
        g, x = g.split(","), x.split(",")
        assert len(g) == len(x) == 15
        for c in range(15):
            if c in SSIM_COLUMNS and x[c] != "nan":
                worst = max(worst, abs(float(g[c]) - float(x[c])))
                assert abs(float(g[c]) - float(x[c])) <= 2 * dist + 1e-9, (what, g[0], c, g[c], x[c], dist)
            else:
                assert g[c] == x[c], (what, g[0], c, g[c], x[c])
    print("%s: %d frames, SSIM cells within %.3e of float64 (bar %.3e)" % (what, n, worst, 2 * dist))
    return rows, dist


def _check_summary(printed, rows, dist):
    """the run's one `gt:` line against gtscore.summary_line of the restatement's rows: every figure formed from integers is the same text, the
    mean SSIM-Y lies within the bar (+ the rounding of its six decimals)"""
    got = [l for l in printed.splitlines() if l.startswith("gt: ") and " frames, PSNR-Y " in l]
    assert len(got) == 1, printed[-2000:]
    g, x = got[0].split(", "), gtscore.summary_line(rows).split(", ")
    assert len(g) == len(x) == 5 and [g[k] for k in (0, 1, 3, 4)] == [x[k] for k in (0, 1, 3, 4)], (g, x)
    assert g[2].startswith("mean SSIM-Y ") and abs(float(g[2].split()[-1]) - float(x[2].split()[-1])) <= 2 * dist + 1e-6, (g, x)


def test_420mpeg2_plain_route_batchings_and_its_own_output_as_ground_truth(tmp_path, ckpt):
    n, H, W = 5, vid.T, vid.T
    chroma = "420mpeg2"
    rs = np.random.RandomState(21)
    blocks = lambda: np.repeat(np.repeat(rs.randint(0, 256, (n, H // 8, W // 8, 3)).astype(np.uint8), 8, axis=1), 8, axis=2)
    to_stream = lambda rgb: vid.ref.y4m_bytes([vid.ref.rgb_to_yuv(x, chroma, "bt601", False) for x in rgb], W, H, chroma,
                                              header=vid.ref.y4m_header(W, H, chroma))
    data, clear = to_stream(blocks()), to_stream(blocks())
    (tmp_path / "in.y4m").write_bytes(data)
    (tmp_path / "clear.y4m").write_bytes(clear)
    runs = {}
    for tag, extra in (("without", ["--batchSize", "2"]), ("b2", ["--batchSize", "2", "--eval_gt", str(tmp_path / "clear.y4m")]),
                       ("b1", ["--batchSize", "1", "--video_buffers", "4", "--eval_gt", str(tmp_path / "clear.y4m")])):
        sub = tmp_path / tag
        sub.mkdir()
        r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", sub / "out.y4m", extra)
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        runs[tag] = (sub, r.stdout.decode())
    out = (runs["without"][0] / "out.y4m").read_bytes()
    assert len(out) == len(data) and out != data
    assert (runs["b2"][0] / "out.y4m").read_bytes() == out and (runs["b1"][0] / "out.y4m").read_bytes() == out
    # without the flag every printed line is what it was: no option line, no summary, no timing entry, no file
    assert not any(l.startswith(("eval_gt", "gt_csv", "gt:")) or "'gt':" in l or "scoring against" in l for l in runs["without"][1].splitlines())
    assert not (runs["without"][0] / "gt.csv").exists()
    csv = (runs["b2"][0] / "gt.csv").read_text()
    assert (runs["b1"][0] / "gt.csv").read_text() == csv          # the batching and the buffers change no cell
    rows, dist = _check_csv(csv, out, clear, H, W, chroma, 8, "plain 420mpeg2")
    for tag in ("b2", "b1"):
        t = runs[tag][1]
        assert "eval_gt: %s" % (tmp_path / "clear.y4m") in t and "gt: wrote %s" % (runs[tag][0] / "gt.csv") in t
        _check_summary(t, rows, dist)
        assert "'gt':" in t.strip().splitlines()[-2]              # the timing line carries the entry
    assert all(r["psnr"][0] < 40 for r in rows) and rows[0]["dt_y"] is None and all(r["dt_y"] > 0 for r in rows[1:])
    # the run's own output as the ground truth: every PSNR is inf, every SSIM 1 and every dt_y 0
    (tmp_path / "own.y4m").write_bytes(out)
    sub = tmp_path / "own"
    sub.mkdir()
    r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", sub / "out.y4m", ["--batchSize", "2", "--eval_gt", str(tmp_path / "own.y4m"), "--gt_csv", str(tmp_path / "own.csv")])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert not (sub / "gt.csv").exists() and (sub / "out.y4m").read_bytes() == out
    lines = (tmp_path / "own.csv").read_text().splitlines()
    assert len(lines) == n + 1
    for k, line in enumerate(lines[1:]):
        c = line.split(",")
        assert c[1:5] == ["inf"] * 4 and c[5:8] == ["1.000000000"] * 3 and c[8] == ("" if k == 0 else "0.000000") and c[9:13] == ["0"] * 4, line
    assert "gt: 5 frames, PSNR-Y inf, mean SSIM-Y 1.000000, PSNR avg inf, mean temporal error 0.0000 levels" in r.stdout.decode()


def test_fit_temporal_route_at_150_x_201(tmp_path, ckpt):
    n, H, W, chroma, flags = vid.CASES["fit"]
    assert (H, W) == (150, 201)
    data, clear = vid._stream("fit")[0], vid._stream("fit", seed=12)[0]
    (tmp_path / "in.y4m").write_bytes(data)
    (tmp_path / "clear.y4m").write_bytes(clear)
    r = deep._run(tmp_path, ckpt, tmp_path / "in.y4m", tmp_path / "out.y4m", flags + ["--temporal", "--eval_gt", str(tmp_path / "clear.y4m")])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "video: temporal stabilisation" in r.stdout.decode()
    _check_csv((tmp_path / "gt.csv").read_text(), (tmp_path / "out.y4m").read_bytes(), clear, H, W, chroma, 8, "fit + temporal")


@pytest.mark.parametrize("route", ["plain", "tile"])
def test_deep_streams_pipe_to_pipe(route, tmp_path, ckpt):
    """C420p10 on the plain route and C444p12 under --tile, with --video_depth auto"""
    n, H, W, chroma, depth, flags = deep.CASES[route]
    data, clear = deep._stream(route)[0], deep._stream(route, seed=12)[0]
    (tmp_path / "clear.y4m").write_bytes(clear)
    plain = deep._run(tmp_path, ckpt, "-", "-", flags, input=data)
    assert plain.returncode == 0, plain.stderr[-3000:]
    r = deep._run(tmp_path, ckpt, "-", "-", flags + ["--eval_gt", str(tmp_path / "clear.y4m"), "--gt_csv", str(tmp_path / "scores.csv")], input=data)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == plain.stdout and len(r.stdout) == len(data)          # nothing but the stream on stdout, and the same stream
    rows, dist = _check_csv((tmp_path / "scores.csv").read_text(), r.stdout, clear, H, W, chroma, depth, "%s %s %d bits" % (route, chroma, depth))
    _check_summary(r.stderr.decode(), rows, dist)
    assert "gt:" not in plain.stderr.decode() and not (tmp_path / "gt.csv").exists()
    if route == "tile":
        # a piped input whose ground truth is one frame short: known only when the frame is reached; the run leaves with 2 naming the frame
        short = clear[:len(clear) - (6 + ref.frame_bytes(H, W, chroma, depth))]
        (tmp_path / "short.y4m").write_bytes(short)
        r = deep._run(tmp_path, ckpt, "-", "-", flags + ["--eval_gt", str(tmp_path / "short.y4m"), "--gt_csv", str(tmp_path / "short.csv")], input=data)
        err = r.stderr.decode()
        assert r.returncode == 2 and "ends before frame %d of the input" % (n - 1) in err and "Traceback" not in err, err[-2000:]
        assert not (tmp_path / "short.csv").exists()


def test_refusals_come_before_the_checkpoint_and_any_output(tmp_path):
    none = tmp_path / "ckpt"                                      # there is no checkpoint: every refusal comes before it is looked for
    n, H, W, chroma, _ = vid.CASES["plain"]
    data, header, frames, _ = vid._stream("plain")
    (tmp_path / "in.y4m").write_bytes(data)
    (tmp_path / "clear.y4m").write_bytes(data)
    other = vid.ref.y4m_bytes([np.zeros(vid.ref.frame_bytes(H, W + 2, chroma), np.uint8)], W + 2, H, chroma)
    (tmp_path / "wider.y4m").write_bytes(other)
    (tmp_path / "mpeg2.y4m").write_bytes(vid.ref.y4m_bytes(frames, W, H, "420mpeg2", header=vid.ref.y4m_header(W, H, "420mpeg2")))
    (tmp_path / "p10.y4m").write_bytes(deep._stream("plain")[0])
    (tmp_path / "short.y4m").write_bytes(data[:len(data) - (6 + vid.ref.frame_bytes(H, W, chroma))])
    dst = tmp_path / "out.y4m"
    for extra, says in ((["--eval_gt", str(tmp_path / "wider.y4m")], "width is %d but the input's is %d" % (W + 2, W)),
                        (["--eval_gt", str(tmp_path / "mpeg2.y4m")], "C tag is C420mpeg2 but the input's is C420jpeg"),
                        (["--eval_gt", str(tmp_path / "p10.y4m"), "--video_depth", "auto"], "C tag is C420p10 but the input's is C420jpeg"),
                        (["--eval_gt", "-"], "- (stdin) is refused"),
                        (["--gt_csv", str(tmp_path / "x.csv")], "needs --eval_gt"),
                        (["--eval_gt", str(tmp_path / "missing.y4m")], "missing.y4m"),
                        (["--eval_gt", str(tmp_path / "short.y4m")], "holds %d frames but the input holds %d: frame %d has no ground truth" % (n - 1, n, n - 1))):
        r = deep._run(tmp_path, none, tmp_path / "in.y4m", dst, extra)
        err = r.stderr.decode()
        assert r.returncode == 2 and says in err and "Traceback" not in err, (extra, r.returncode, err[-2000:])
        assert not dst.exists() and not (tmp_path / "gt.csv").exists() and not (tmp_path / "x.csv").exists()
    r = deep._run(tmp_path, none, tmp_path / "in.y4m", "-", ["--eval_gt", str(tmp_path / "clear.y4m")])
    assert r.returncode == 2 and r.stdout == b"" and "--gt_csv PATH" in r.stderr.decode()
    # a piped input: the headers are compared once the input's is read; nothing on stdout
    r = deep._run(tmp_path, none, "-", "-", ["--eval_gt", str(tmp_path / "wider.y4m"), "--gt_csv", str(tmp_path / "x.csv")], input=data)
    assert r.returncode == 2 and r.stdout == b"" and "width is %d but the input's is %d" % (W + 2, W) in r.stderr.decode()
    assert not (tmp_path / "x.csv").exists()
