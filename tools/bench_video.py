#!/usr/bin/env python3
"""Stream-to-stream throughput of dehaze_video.py against the PNG route of test.py on the same pictures, in the same run on the same box:

    python tools/bench_video.py [--frames 512] [--out profiles/video_throughput.json]

Writes `frames` synthetic 512 x 512 pictures (the ones tools/cli_throughput.py uses) as PNGs and, converted with the integer tables of
cfen_vit_dehazing_amd/yuv.py (bt601 limited, 2 x 2 means for the chroma), as one 420jpeg .y4m file on local disk, plus a seeded checkpoint; then times
  video      python dehaze_video.py --precision half --batchSize 8, file to file, the plain route: the `video: N frames in S s` line
  png        python test.py --precision half --u8_input --batchSize 8 --in_flight 4 --nThreads T --writers W --gpu_png on the PNGs: the
             `images/s file to file` line of the pipelined driver
  forward    python bench.py --gpus 1 --in-flight 1: the one-forward-at-a-time rate, the GPU alone
Every leg is a child process under its own time limit; a leg that fails or runs over stops the tool.  Prints / writes ONE JSON object."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEG_TIMEOUT_S = 400


def _leg(cmd, cwd, env=None):
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LEG_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        raise SystemExit("%s ran over its %d s limit: stopping" % (os.path.basename(cmd[1]), LEG_TIMEOUT_S))
    if p.returncode != 0:
        raise SystemExit("%s failed (exit %d): stopping\n%s" % (os.path.basename(cmd[1]), p.returncode, p.stdout[-2000:]))
    return p.stdout, round(time.perf_counter() - t0, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "video_throughput.json"))
    ap.add_argument("--bench-steps", type=int, default=50)
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from cfen_vit_dehazing_amd import yuv
    from cfen_vit_dehazing_amd.config import NetConfig
    from cfen_vit_dehazing_amd.manifest import generate_state_dict
    ncpu = len(os.sched_getaffinity(0))
    threads, writers = min(16, max(2, ncpu // 2)), min(32, max(4, ncpu // 2))
    tmp = tempfile.mkdtemp(prefix="cfen_video_")
    try:
        name = "iid_hlgvit_crs_gd4_cfs_v3_video"
        os.makedirs(os.path.join(tmp, "ckpt", name))
        torch.save(generate_state_dict(NetConfig(24, 4, patch_size=32, load_size=256), seed=0), os.path.join(tmp, "ckpt", name, "32_net_G.pth"))
        hazy = os.path.join(tmp, "data", "hazy")
        os.makedirs(hazy)
        rs = np.random.RandomState(1)
        n = 512
        yy, xx = np.mgrid[0:n, 0:n].astype(np.float32) / n
        fwd, _, oy = yuv.tables("bt601", False)
        fwd = fwd.astype(np.int64)
        with open(os.path.join(tmp, "in.y4m"), "wb") as f:
            f.write(b"YUV4MPEG2 W512 H512 F25:1 Ip A1:1 C420jpeg\n")
            for i in range(args.frames):
                base = np.stack([np.sin(6.0 * (xx * (i % 5 + 1) + yy)) * 90 + 128, np.cos(5.0 * (yy * (i % 3 + 1) - xx)) * 80 + 120, (xx + yy) * 100 + 20 + (i % 50)], -1)
                img = np.clip(base + rs.randn(n, n, 3) * 6.0, 0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(hazy, "syn_%05d.png" % i))
                d = np.clip((img.astype(np.int64) @ fwd.T + (np.array([oy, 128, 128]) << 14) + 8192) >> 14, 0, 255)
                c = (d[0::2, 0::2, 1:] + d[0::2, 1::2, 1:] + d[1::2, 0::2, 1:] + d[1::2, 1::2, 1:] + 2) >> 2
                f.write(b"FRAME\n" + d[..., 0].astype(np.uint8).tobytes() + c[..., 0].astype(np.uint8).tobytes() + c[..., 1].astype(np.uint8).tobytes())
        model = ["--name", name, "--n_feats", "24", "--hidden_dim_ratio", "4", "--which_epoch", "32", "--checkpoints_dir", os.path.join(tmp, "ckpt"),
                 "--precision", "half", "--batchSize", "8"]
        res = {"frames": args.frames, "frame": "512x512 420jpeg", "usable_cpus": ncpu, "decode_workers": threads, "writer_threads": writers,
               "y4m_bytes": os.path.getsize(os.path.join(tmp, "in.y4m")),
               "png_bytes": sum(os.path.getsize(os.path.join(hazy, p)) for p in os.listdir(hazy))}
        # ---- the video route ------------------------------------------------------------------------------------------------------------
        out, wall = _leg([sys.executable, os.path.join(ROOT, "dehaze_video.py"), "--in", os.path.join(tmp, "in.y4m"), "--out", os.path.join(tmp, "out.y4m")] + model, tmp)
        m = re.search(r"video: (\d+) frames in ([0-9.]+) s = ([0-9.]+) frames/s stream to stream", out)
        mt = re.search(r"main-thread seconds (\{.*\})", out)
        if not m or int(m.group(1)) != args.frames or os.path.getsize(os.path.join(tmp, "out.y4m")) != res["y4m_bytes"]:
            raise SystemExit("dehaze_video.py did not write %d frames: stopping\n%s" % (args.frames, out[-2000:]))
        res["video"] = {"frames_per_s_stream_to_stream": float(m.group(3)), "loop_seconds": float(m.group(2)),
                        "main_thread_seconds": json.loads(mt.group(1).replace("'", '"')) if mt else None, "process_wall_seconds": wall,
                        "flags": "--precision half --batchSize 8 (--video_buffers 4)"}
        # ---- the PNG route --------------------------------------------------------------------------------------------------------------
        # the PNG leg is the parent's best configuration, as tools/cli_throughput.py measures it: without a caller's GPU_MAX_HW_QUEUES test.py sets
        # 8 for its four streams.  The other two legs use one stream and run under whatever the caller's environment says; all three are recorded
        env = dict(os.environ)
        env.pop("GPU_MAX_HW_QUEUES", None)
        inherited = os.environ.get("GPU_MAX_HW_QUEUES", "unset (the runtime's default, 4)")
        res["gpu_max_hw_queues"] = {"video": inherited + ", one stream", "png": "8, set by test.py for --in_flight 4 (the caller's value removed)",
                                    "forward": inherited + ", one stream"}
        extra = ["--in_flight", "4", "--nThreads", str(threads), "--writers", str(writers), "--gpu_png"]
        out, wall = _leg([sys.executable, os.path.join(ROOT, "test.py"), "--dataroot", os.path.join(tmp, "data"), "--sb", "--out_all", "--u8_input",
                          "--results_dir", os.path.join(tmp, "res")] + model + extra, tmp, env)
        m = re.search(r"(\d+) images in ([0-9.]+) s = ([0-9.]+) images/s file to file", out)
        mt = re.search(r"main-thread seconds (\{.*\})", out)
        if not m or int(m.group(1)) != args.frames:
            raise SystemExit("test.py did not write %d images: stopping\n%s" % (args.frames, out[-2000:]))
        res["png"] = {"images_per_s_file_to_file": float(m.group(3)), "loop_seconds": float(m.group(2)),
                      "main_thread_seconds": json.loads(mt.group(1).replace("'", '"')) if mt else None, "process_wall_seconds": wall,
                      "flags": "--precision half --u8_input --batchSize 8 " + " ".join(extra)}
        # ---- the GPU alone --------------------------------------------------------------------------------------------------------------
        out, wall = _leg([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", "5", "--in-flight", "1",
                          "--no-cpu-baseline", "--no-extra-configs"], tmp)
        line = [l for l in out.splitlines() if l.startswith("{")][-1]
        b = json.loads(line)
        if b["pipelining"]["forwards_in_flight"] != 1:
            raise SystemExit("bench.py --in-flight 1 reported %s forwards in flight: stopping" % b["pipelining"]["forwards_in_flight"])
        res["forward"] = {"images_per_s_one_forward_at_a_time": b["value"], "ms_per_step": b["ms_per_step"], "graph": b["config"]["graph"],
                          "flags": "--gpus 1 --steps %d --warmup 5 --in-flight 1" % args.bench_steps}
        v, p, g = res["video"]["frames_per_s_stream_to_stream"], res["png"]["images_per_s_file_to_file"], res["forward"]["images_per_s_one_forward_at_a_time"]
        res["video_over_png"] = round(v / p, 3)
        res["video_share_of_one_forward_at_a_time"] = round(v / g, 3)
        mts = res["video"]["main_thread_seconds"] or {}
        res["bound"] = ("the video loop's main thread spent %.2f s waiting for frames and %.2f s issuing device work of %.2f s in all"
                        % (mts.get("wait_for_frames", float("nan")), mts.get("issue", float("nan")), res["video"]["loop_seconds"]))
        print(json.dumps(res))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
