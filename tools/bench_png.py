#!/usr/bin/env python3
"""Device time and output size of the device PNG encoder (cfen_png_deflate; cfen_vit_dehazing_amd/png.py):

    python3 tools/bench_png.py [out_time.json] [out_size.json]

time  eight 512 x 512 images in one call and one 2160 x 3840 image: events around `reps` back-to-back calls, repeated `runs` times, the median run's
      time per call; beside it the batch-8 fp16 forward on the same stream, alone and followed by the encode of its fake_A bytes.
size  total IDAT bytes of the encoder against two baselines over the SAME filtered scanlines (tests/png_ref.filtered_scanlines):
      zlib Z_HUFFMAN_ONLY -- an optimal per-stream Huffman code without matching, the floor of this design -- and PIL's default file;
      on the dehazed outputs of the seeded bench inputs and on the test image generators.
Prints one JSON object per part."""
import io
import json
import os
import statistics
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from PIL import Image

import metrics_images
import png_ref
from cfen_vit_dehazing_amd import ops, png
from cfen_vit_dehazing_amd.config import NetConfig
from cfen_vit_dehazing_amd.hipnet import dec_ipt
from cfen_vit_dehazing_amd.manifest import generate_state_dict, synthetic_input

DEV = "cuda:0"


def timed(fn, reps=20, runs=7):
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
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "reps": reps, "runs": runs}


def sizes(images):
    """bytes of (device encoder's IDAT payload, Z_HUFFMAN_ONLY of the same filtered bytes, PIL's default IDAT payloads) summed over the images"""
    t = torch.from_numpy(np.ascontiguousarray(images)).to(DEV)
    lengths = ops.png_deflate(t)[1].cpu().numpy()
    ours = int(lengths.sum())
    huff = pil = 0
    for img in images:
        c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
        lines = png_ref.filtered_scanlines(img).tobytes()
        huff += len(c.compress(lines) + c.flush())
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        pil += len(buf.getvalue()) - 57                                  # signature 8, IHDR 25, IDAT framing 12, IEND 12
    return {"images": len(images), "raw_bytes": int(images.size), "device_idat_bytes": ours, "huffman_only_bytes": huff, "pil_default_idat_bytes": pil,
            "device_over_huffman_only": round(ours / huff, 4), "device_over_pil_default": round(ours / pil, 4)}


def main():
    out_time = sys.argv[1] if len(sys.argv) > 1 else None
    out_size = sys.argv[2] if len(sys.argv) > 2 else None
    cfg = NetConfig(24, 4, patch_size=32, load_size=256)               # 512 x 512, the bench configuration
    net = dec_ipt(cfg, compute_dtype="fp16")
    net.load_state_dict(generate_state_dict(cfg, seed=0), strict=True)
    net.to(DEV)
    net.output_u8 = True
    x = synthetic_input(8, cfg).to(DEV)
    with torch.no_grad():
        fake_a = net(x)[2].clone()
    torch.cuda.synchronize()
    assert fake_a.dtype == torch.uint8 and tuple(fake_a.shape) == (8, 512, 512, 3)

    big = torch.from_numpy(png_ref.smooth(2160, 3840, 8)[None]).to(DEV)
    slab8, len8 = ops.png_deflate(fake_a)
    slabb, lenb = ops.png_deflate(big)
    res_t = {"device": torch.cuda.get_device_name(0),
             "encode_8x512x512_forward_outputs": timed(lambda: ops.png_deflate(fake_a, slab8, len8)),
             "encode_1x2160x3840": timed(lambda: ops.png_deflate(big, slabb, lenb), reps=5)}
    with torch.no_grad():
        res_t["forward_batch8_fp16_eager_one_stream"] = timed(lambda: net(x))
        res_t["forward_then_encode_one_stream"] = timed(lambda: ops.png_deflate(net(x)[2], slab8, len8))
    f, fe = res_t["forward_batch8_fp16_eager_one_stream"]["median_ms"], res_t["forward_then_encode_one_stream"]["median_ms"]
    res_t["images_per_s_forward_only"] = round(8000.0 / f, 1)
    res_t["images_per_s_forward_then_encode"] = round(8000.0 / fe, 1)
    res_t["note"] = ("one stream, eager launches: the encode's device time adds to the forward's; the four-in-flight graph replay of bench.py is measured file to "
                     "file by tools/cli_throughput.py (pipelined_gpu_png)")
    print(json.dumps(res_t))

    res_s = {"forward_outputs_seeded_bench_inputs_8x512x512": sizes(fake_a.cpu().numpy())}
    for name in ("512x512_batch8", "480x640", "1080x1920"):
        res_s["metrics_images_" + name] = sizes(metrics_images.pair(name)[0])
    res_s["smooth_2160x3840"] = sizes(png_ref.smooth(2160, 3840, 8)[None])
    print(json.dumps(res_s))
    for path, res in ((out_time, res_t), (out_size, res_s)):
        if path:
            with open(path, "w") as fh:
                json.dump(res, fh, indent=1, sort_keys=True)
                fh.write("\n")


if __name__ == "__main__":
    main()
