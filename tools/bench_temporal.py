#!/usr/bin/env python3
"""Device time of temporal stabilisation (cfen_temporal_blend + cfen_temporal_apply_u8; csrc/k_temporal.hip, include/cfen_temporal.h), and what
--temporal costs dehaze_video.py stream to stream:

    python3 tools/bench_temporal.py [out.json] [--ops-only] [--frames 256]         (default profiles/temporal_bench.json)

ops       for eight 512 x 512 frames (down = auto = 1: the working resolution is the frame, k_temporal_apply's global-memory path) and for one
          2160 x 3840 frame (down = auto = 4: 540 x 960, the staged path): ops.temporal_blend and ops.temporal_apply_u8, the whole
          Stabiliser.step around them (box resample where down > 1, guided_coef_u8, the copy of the last working frame), and beside them, in the
          same run, ops.guided_apply_u8 on the same coefficient and frame sizes and a device copy of the frames' bytes.  Events around `reps`
          back-to-back calls, the median of 7 runs.  Bytes moved by the apply kernel (hazy and dehazed read, output written, delta read once)
          and their rate as a share of the 6.29 TB/s copy rate DESIGN uses.
video     python dehaze_video.py --precision half --batchSize 8 on a synthetic 512 x 512 420jpeg stream (the pictures of tools/bench_video.py),
          file to file, without and with --temporal: the `video: N frames in S s` line of each child process.  --ops-only leaves this part out.
Prints the JSON object it writes."""
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from cfen_vit_dehazing_amd import ops, temporal

DEV = "cuda:0"
COPY_RATE = 6.29e12          # bytes / s, the device copy rate of DESIGN section 6
LEG_TIMEOUT_S = 300


def timed(fn, reps=50, runs=7):
    """median over `runs` of the time per call in ms of `reps` back-to-back calls between two events"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), min(out), max(out)


def us(t):
    return {"device_us": round(t[0] * 1e3, 2), "device_us_min_max": [round(t[1] * 1e3, 2), round(t[2] * 1e3, 2)]}


def ops_case(n, H, W, seed):
    S, h, w = temporal.working_size(H, W)
    rs = np.random.RandomState(seed)
    G = torch.from_numpy(rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)).to(DEV)
    Y = torch.from_numpy(np.clip(rs.randint(0, 256, (n, H, W, 3)) * 0.8 + 20, 0, 255).astype(np.uint8)).to(DEV)
    I, P = (G, Y) if S == 1 else (ops.resample_u8(G, (h, w), filter="box"), ops.resample_u8(Y, (h, w), filter="box"))
    coef = ops.guided_coef_u8(I, P, 2)
    state = torch.zeros(h, w, 6, device=DEV)
    prev = I[0].clone()
    delta = torch.empty(n, h, w, 6, device=DEV)
    out = torch.empty_like(G)
    res = {"case": "%d x %dx%d, working resolution %dx%d (down = auto = %d), radius 2" % (n, H, W, h, w, S)}
    res["temporal_blend (k_temporal_blend)"] = us(timed(lambda: ops.temporal_blend(I, prev, coef, state, 2, 8.0, 0.8, True, out=delta)))
    for name, fn, planes in (("temporal_apply_u8 (k_temporal_apply)", lambda: ops.temporal_apply_u8(delta, G, Y, out=out), 3),
                             ("guided_apply_u8 (k_guided_apply), same sizes", lambda: ops.guided_apply_u8(coef, G, out=out), 2)):
        t = timed(fn)
        moved = planes * n * H * W * 3 + n * h * w * 24
        res[name] = dict(us(t), bytes_moved=moved, share_of_copy_rate=round(moved / (t[0] * 1e-3) / COPY_RATE, 4))
    t = timed(lambda: out.copy_(G))
    res["device copy of the frames"] = dict(us(t), bytes_moved=2 * n * H * W * 3, share_of_copy_rate=round(2 * n * H * W * 3 / (t[0] * 1e-3) / COPY_RATE, 4))
    st = temporal.Stabiliser()
    st.step(G, Y)
    res["Stabiliser.step (resample + guided_coef_u8 + blend + copy + apply)"] = us(timed(lambda: st.step(G, Y, out=out)))
    return res


def write_clip(path, frames):
    """the pictures of tools/bench_video.py as one 420jpeg stream (bt601 limited, 2 x 2 means for the chroma)"""
    from cfen_vit_dehazing_amd import yuv
    rs = np.random.RandomState(1)
    n = 512
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float32) / n
    fwd, _, oy = yuv.tables("bt601", False)
    fwd = fwd.astype(np.int64)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W512 H512 F25:1 Ip A1:1 C420jpeg\n")
        for i in range(frames):
            base = np.stack([np.sin(6.0 * (xx * (i % 5 + 1) + yy)) * 90 + 128, np.cos(5.0 * (yy * (i % 3 + 1) - xx)) * 80 + 120, (xx + yy) * 100 + 20 + (i % 50)], -1)
            img = np.clip(base + rs.randn(n, n, 3) * 6.0, 0, 255).astype(np.uint8)
            d = np.clip((img.astype(np.int64) @ fwd.T + (np.array([oy, 128, 128]) << 14) + 8192) >> 14, 0, 255)
            c = (d[0::2, 0::2, 1:] + d[0::2, 1::2, 1:] + d[1::2, 0::2, 1:] + d[1::2, 1::2, 1:] + 2) >> 2
            f.write(b"FRAME\n" + d[..., 0].astype(np.uint8).tobytes() + c[..., 0].astype(np.uint8).tobytes() + c[..., 1].astype(np.uint8).tobytes())


def video_legs(frames):
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.manifest import generate_state_dict
    tmp = tempfile.mkdtemp(prefix="cfen_temporal_")
    try:
        name = "iid_hlgvit_crs_gd4_cfs_v3_video"
        os.makedirs(os.path.join(tmp, "ckpt", name))
        torch.save(generate_state_dict(NetConfig(24, 4, patch_size=32, load_size=256), seed=0), os.path.join(tmp, "ckpt", name, "32_net_G.pth"))
        write_clip(os.path.join(tmp, "in.y4m"), frames)
        model = ["--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4", "--which_epoch", "32", "--checkpoints_dir", os.path.join(tmp, "ckpt"),
                 "--precision", "half", "--batchSize", "8"]
        res = {"frames": frames, "frame": "512x512 420jpeg", "flags": "--precision half --batchSize 8 (--video_buffers 4)"}
        for leg, extra in (("without", []), ("with --temporal", ["--temporal"]), ("without, again", [])):
            cmd = [sys.executable, os.path.join(ROOT, "dehaze_video.py"), "--in", os.path.join(tmp, "in.y4m"), "--out", os.path.join(tmp, "out.y4m")] + model + extra
            try:
                p = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LEG_TIMEOUT_S)
            except subprocess.TimeoutExpired:
                raise SystemExit("dehaze_video.py (%s) ran over its %d s limit: stopping" % (leg, LEG_TIMEOUT_S))
            m = re.search(r"video: (\d+) frames in ([0-9.]+) s = ([0-9.]+) frames/s stream to stream", p.stdout)
            if p.returncode != 0 or not m or int(m.group(1)) != frames:
                raise SystemExit("dehaze_video.py (%s) failed (exit %d): stopping\n%s" % (leg, p.returncode, p.stdout[-2000:]))
            mt = re.search(r"main-thread seconds (\{.*\})", p.stdout)
            res[leg] = {"frames_per_s_stream_to_stream": float(m.group(3)), "loop_seconds": float(m.group(2)),
                        "main_thread_seconds": json.loads(mt.group(1).replace("'", '"')) if mt else None}
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    args = [a for a in sys.argv[1:] if a != "--ops-only"]
    frames = 256
    if "--frames" in args:
        i = args.index("--frames")
        frames = int(args[i + 1])
        del args[i:i + 2]
    out_path = args[0] if args else os.path.join(ROOT, "profiles", "temporal_bench.json")
    res = {"device": torch.cuda.get_device_name(0), "timing": "device events, 50 calls per run, median of 7 runs"}
    res["8 x 512x512"] = ops_case(8, 512, 512, 3)
    print(json.dumps(res["8 x 512x512"]), flush=True)
    res["1 x 2160x3840"] = ops_case(1, 2160, 3840, 4)
    print(json.dumps(res["1 x 2160x3840"]), flush=True)
    if "--ops-only" not in sys.argv:
        torch.cuda.synchronize()
        res["dehaze_video.py"] = video_legs(frames)
        print(json.dumps(res["dehaze_video.py"]), flush=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
