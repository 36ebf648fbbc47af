"""Images/s of the two ways to turn JPEG files into the captioner's input tensor:

    host    PIL decode (one thread) + DevicePreprocessor.__call__ (upload RGB, resize + normalise on the GPU)
    device  DevicePreprocessor.from_jpeg_bytes (upload the compressed bytes, odic_jpeg_decode, resize + normalise)

Inputs: 640x480 q90 4:2:0 JPEGs with photo statistics, re-encoded at run time from crops and resizes of
tests/golden/demo_material/micheal.jpg.  Both paths are timed in the same process, alternating, at each batch
size; the two results are checked torch.equal first.  One JSON line per batch size goes to stdout and --out.

    python tools/jpeg_bench.py --batches 16 64 --iters 20 --out profiles/r04_jpeg_bench.json
    python tools/jpeg_bench.py --device-only --batches 64 --iters 5      # under rocprofv3 --kernel-trace --stats
    python tools/jpeg_bench.py --progressive --out profiles/r05_jpeg_progressive_bench.json

--progressive: the same crops saved with progressive=True (libjpeg's standard ten-scan script), for which the host
path is what every progressive file took before odic_jpeg_decode_progressive; then tatin.jpg itself (1280x960), alone
and as a batch of copies; and the cost of jpeg.parse_progressive per file.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(n: int, seed: int = 0, progressive: bool = False):
    from PIL import Image
    src = Image.open(os.path.join(ROOT, "tests", "golden", "demo_material", "micheal.jpg")).convert("RGB")
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w = int(rng.integers(360, src.width))
        h = int(rng.integers(int(w * 0.6), min(src.height, int(w * 0.9)) + 1))
        x, y = int(rng.integers(0, src.width - w + 1)), int(rng.integers(0, src.height - h + 1))
        im = src.crop((x, y, x + w, y + h)).resize((640, 480), Image.BICUBIC)
        if rng.integers(2):
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        buf = io.BytesIO()
        im.save(buf, format="JPEG", quality=90, subsampling=2, progressive=progressive)
        out.append(buf.getvalue())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="also time the device path at other subseq_bits / passes")
    ap.add_argument("--progressive", action="store_true", help="progressive re-saves of the crops, and tatin.jpg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    pre = DevicePreprocessor(args.size, "cuda:0")
    blobs_all = make_inputs(max(args.batches), progressive=args.progressive)
    want_route = "device-progressive" if args.progressive else "device"
    inputs = [(B, blobs_all[:B], (640, 480)) for B in args.batches]
    parse_us = None
    if args.progressive:
        from on_device_image_captioning_amd import jpeg as J
        with open(os.path.join(ROOT, "tests", "golden", "demo_material", "tatin.jpg"), "rb") as f:
            tatin = f.read()
        inputs += [(1, [tatin], (1280, 960)), (16, [tatin] * 16, (1280, 960))]
        t0 = time.perf_counter()
        for _ in range(5):
            for b in blobs_all:
                J.parse(b)
                J.parse_progressive(b)
        parse_us = 1e6 * (time.perf_counter() - t0) / (5 * len(blobs_all))

    def host(blobs):
        return pre([np.asarray(Image.open(io.BytesIO(b))) for b in blobs])

    def device(blobs):
        return pre.from_jpeg_bytes(blobs, progressive="device" if args.progressive else "host")

    lines = []
    for B, blobs, (width, height) in inputs:
        if args.device_only:
            for _ in range(args.warmup + args.iters):
                device(blobs)
            torch.cuda.synchronize()
            continue
        assert torch.equal(host(blobs), device(blobs)), "host and device paths differ"
        assert set(pre.last_routes) == {want_route}, pre.last_routes
        for _ in range(args.warmup):
            host(blobs)
            device(blobs)
        torch.cuda.synchronize()
        t = {"host": [], "device": []}
        for _ in range(args.iters):
            for name, fn in (("host", host), ("device", device)):
                t0 = time.perf_counter()
                fn(blobs)
                torch.cuda.synchronize()
                t[name].append(time.perf_counter() - t0)
        med = {k: float(np.median(v)) for k, v in t.items()}
        sweep = {}
        if args.sweep:
            for bits in (1024, 2048, 4096):
                for passes in (2, 4, 8):
                    fn = lambda b, bits=bits, passes=passes: pre.from_jpeg_bytes(b, bits, passes)   # noqa: E731
                    for _ in range(2):
                        fn(blobs)
                    torch.cuda.synchronize()
                    ts = []
                    for _ in range(args.iters):
                        t0 = time.perf_counter()
                        fn(blobs)
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t0)
                    sweep[f"bits{bits}_passes{passes}"] = B / float(np.median(ts))
        line = {"batch": B, "width": width, "height": height, "quality": 90, "subsampling": "4:2:0",
                "progressive": args.progressive,
                "mean_jpeg_bytes": int(np.mean([len(b) for b in blobs])),
                "host_images_per_s": B / med["host"], "device_images_per_s": B / med["device"],
                "speedup": med["host"] / med["device"],
                "host_ms_median": 1e3 * med["host"], "device_ms_median": 1e3 * med["device"],
                "host_ms_min": 1e3 * min(t["host"]), "device_ms_min": 1e3 * min(t["device"]), "iters": args.iters,
                "gpu": torch.cuda.get_device_name(0)}
        if parse_us is not None:
            line["parse_plus_parse_progressive_us_per_640x480_file"] = parse_us
        if sweep:
            line["device_images_per_s_sweep"] = sweep
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
