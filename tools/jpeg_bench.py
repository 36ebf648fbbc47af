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

--gray: the same crops saved as mode L (one component), decoded under non_rgb="convert": the device path against the
host's `Image.open(f).convert("RGB")`; with --progressive, their progressive re-saves.

    python tools/jpeg_bench.py --gray --batches 16 64 --iters 20 --out profiles/r12_jpeg_gray_bench.json

--cmyk: the same crops saved as mode CMYK (four components; Pillow writes Adobe transform 0 with component 0 at 2x2 for
subsampling=2), decoded under non_rgb="convert": the device path with cmyk="device" (odic_jpeg_any_decode) against the
host's `Image.open(f).convert("RGB")`.  This is the line that decides whether cmyk="device" becomes the default
(DESIGN §4.25).

    python tools/jpeg_bench.py --cmyk --batches 16 64 --iters 20 --out profiles/jpeg_cmyk_bench.json

--layouts: 640x480 gradient-plus-noise pictures written at 4:4:0 and 4:1:1 by the tests' writer (Pillow's encoder cannot),
eight distinct files per layout repeated to the batch size: the device path with layouts="all" (odic_jpeg_any_decode)
against the host's `Image.open(f).convert("RGB")` on one thread.  One line per layout and batch.

    python tools/jpeg_bench.py --layouts --batches 16 64 --iters 20 --out profiles/jpeg_layouts_bench.json

--progressive-layouts: the two progressive routes with per-component sampling: 640x480 pictures written
as progressive 4:4:0 by the tests' writer (four distinct files, repeated) and the crops saved by Pillow as progressive
CMYK; the device path with progressive="device", cmyk="device", layouts="all" (odic_jpeg_decode_progressive_any)
against the host's `Image.open(f).convert("RGB")` on one thread.  One line per kind and batch.

    python tools/jpeg_bench.py --progressive-layouts --batches 16 64 --iters 20

--draft: what decoding at the scale `Image.draft("RGB", (S, S))` picks saves.  Seeded synthetic JPEGs,
3456x4608 (drafts at 1/8) and 640x480 (drafts at 1/1: the control), 4:2:0 and 4:4:4, baseline and progressive; per
case `decode_jpeg` alone and `from_jpeg_bytes` (decode + resize), draft off and on alternating in the same process,
median / quartiles / min over --iters.  The drafted pixels are checked against Pillow's first.  The per-kernel split
comes from a profiler run of its own (tools/jpeg_sync_stats.py is a CPU model of the synchronisation and times no
kernel), in which the scaled kernels carry their own names; profiles/r11_jpeg_draft_kernel_stats.txt is its table:

    python tools/jpeg_bench.py --draft --iters 15 --warmup 3 --out profiles/r11_jpeg_draft_bench.json
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/jpeg_bench.py --draft --device-only --draft-cases large \
        --iters 4 --warmup 1

--draft-layouts: the draft request on the files of cmyk="device" / layouts="all" (DESIGN §4.28): a batch of four
3456x4608 CMYK files from Pillow's encoder (drafts at 1/8) and a batch of four 2048x1536 4:4:0 files from the tests'
writer (two distinct pictures; drafts at 1/4), each decoded by `decode_jpeg(draft=(S, S))` and by `from_jpeg_bytes(draft=
True)` with draft_layouts="common" (PIL decodes them, one thread) and draft_layouts="all" (the _scaled entry points),
alternating in the same process; the two results are checked torch.equal first.

    python tools/jpeg_bench.py --draft-layouts --iters 10 --warmup 2 --out profiles/jpeg_draft_layouts_bench.json

--orient: EXIF orientation.  First odic_orient_rgb8 alone, device events around a run of launches, for
each of the seven orientations at 4032x3024 and 640x480 (one image, and the batch of 16 the end-to-end case launches),
next to `torch.Tensor.copy_` of the same bytes between two uint8 device buffers: the copy moves each byte once in and
once out, as the kernel does.  Then a batch of 16 640x480 files tagged orientation 6, three ways, alternating:
`from_files(decode="host", orientation="exif")`, `from_jpeg_bytes(orientation="exif")` and
`from_jpeg_bytes()` (orientation ignored) on the same files.

    python tools/jpeg_bench.py --orient --iters 20 --out profiles/r22_jpeg_orient_bench.json
"""
from __future__ import annotations

import argparse
import functools
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(n: int, seed: int = 0, progressive: bool = False, gray: bool = False, cmyk: bool = False):
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
        if gray:
            im.convert("L").save(buf, format="JPEG", quality=90, progressive=progressive)
        elif cmyk:
            im.convert("CMYK").save(buf, format="JPEG", quality=90, subsampling=2, progressive=progressive)
        else:
            im.save(buf, format="JPEG", quality=90, subsampling=2, progressive=progressive)
        out.append(buf.getvalue())
    return out


@functools.lru_cache(maxsize=None)
def layout_inputs(layout: str, n: int, distinct: int = 8):
    """n files of 640x480 at `layout` (a key of tests/jpeg_layout_cases.LAYOUTS): `distinct` pictures, repeated."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from jpeg_layout_cases import LAYOUTS, picture
    from jpeg_layout_writer import write_jpeg3
    hv, style = LAYOUTS[layout]
    files = [write_jpeg3(picture(480, 640, seed=k, noise=True), hv, style) for k in range(min(n, distinct))]
    return [files[k % len(files)] for k in range(n)]


@functools.lru_cache(maxsize=None)
def progressive_layout_inputs(layout: str, n: int, distinct: int = 4):
    """n progressive files of 640x480 at `layout` (a key of tests/jpeg_prog_layout_cases.LAYOUTS) under libjpeg's
    standard script: `distinct` pictures, repeated."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from jpeg_prog_layout_cases import LAYOUTS, source
    from jpeg_prog_layout_writer import standard_script, write_progressive_any, zigzag_coefficients
    hv, style = LAYOUTS[layout]
    files = []
    for k in range(min(n, distinct)):
        zz, _, _ = zigzag_coefficients(source(len(hv), 480, 640, seed=k, noise=True), hv, 6)
        files.append(write_progressive_any(640, 480, hv, zz, 6, standard_script(len(hv)), style))
    return [files[k % len(files)] for k in range(n)]


def synthetic_rgb(h: int, w: int, seed: int) -> np.ndarray:
    """A seeded image with a photograph's spectrum, roughly: smooth fields at three scales plus sensor-like noise."""
    from PIL import Image
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 3), np.float32)
    for div, amp in ((64, 70.0), (16, 30.0), (4, 12.0)):
        small = rng.normal(0, 1, (max(h // div, 2), max(w // div, 2), 3)).astype(np.float32)
        for c in range(3):
            img[:, :, c] += amp * np.asarray(Image.fromarray(small[:, :, c]).resize((w, h), Image.BICUBIC))
    img += 128 + rng.normal(0, 3, img.shape).astype(np.float32)
    return np.clip(img, 0, 255).astype(np.uint8)


DRAFT_CASES = [(size, batch, sub, prog) for size, batch in (((3456, 4608), 4), ((640, 480), 16))
               for sub in (2, 0) for prog in (False, True)]


def draft_bench(args):
    """Draft off against draft on: the same build, the same files, alternating."""
    import torch
    from PIL import Image
    from on_device_image_captioning_amd import jpeg as J
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    S = args.size
    pre = DevicePreprocessor(S, "cuda:0")
    lines = []
    for (w, h), B, sub, prog in DRAFT_CASES:
        if args.draft_cases == "large" and w < 1000:
            continue
        blobs = []
        for k in range(B):
            buf = io.BytesIO()
            Image.fromarray(synthetic_rgb(h, w, seed=k)).save(buf, format="JPEG", quality=90, subsampling=sub,
                                                              progressive=prog)
            blobs.append(buf.getvalue())
        route = "device" if prog else "host"
        fns = {"decode": lambda d: pre.decode_jpeg(blobs, progressive=route, draft=(S, S) if d else None),
               "decode_resize": lambda d: pre.from_jpeg_bytes(blobs, progressive=route, draft=d)}
        if args.device_only:
            for _ in range(args.warmup + args.iters):
                for d in (False, True):
                    fns["decode_resize"](d)
            torch.cuda.synchronize()
            continue
        scale = J.draft_scale((w, h), (S, S))
        im = Image.open(io.BytesIO(blobs[0]))
        im.draft("RGB", (S, S))
        got = fns["decode"](True)[0]
        assert pre.last_routes == ("device-progressive" if prog else "device",) * B, pre.last_routes
        assert torch.equal(got.cpu(), torch.from_numpy(np.asarray(im).copy())), "drafted decode differs from Pillow"
        line = {"width": w, "height": h, "batch": B, "quality": 90, "subsampling": {2: "4:2:0", 0: "4:4:4"}[sub],
                "progressive": prog, "draft_scale": scale, "drafted_size": list(J.scaled_size((w, h), scale)),
                "mean_jpeg_bytes": int(np.mean([len(b) for b in blobs])), "iters": args.iters,
                "gpu": torch.cuda.get_device_name(0)}
        for name, fn in fns.items():
            for _ in range(args.warmup):
                fn(False)
                fn(True)
            torch.cuda.synchronize()
            t = {False: [], True: []}
            for _ in range(args.iters):
                for d in (False, True):
                    t0 = time.perf_counter()
                    fn(d)
                    torch.cuda.synchronize()
                    t[d].append(1e3 * (time.perf_counter() - t0))
            for d, key in ((False, "full"), (True, "draft")):
                q1, med, q3 = (float(x) for x in np.percentile(t[d], [25, 50, 75]))
                line[f"{name}_{key}_ms"] = {"median": med, "q1": q1, "q3": q3, "min": float(min(t[d]))}
            line[f"{name}_full_over_draft"] = line[f"{name}_full_ms"]["median"] / line[f"{name}_draft_ms"]["median"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def draft_layouts_bench(args):
    """draft_layouts="common" against "all" under a draft request: the same build, the same files, alternating."""
    import torch
    from PIL import Image
    from on_device_image_captioning_amd import jpeg as J
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from jpeg_layout_cases import LAYOUTS, picture
    from jpeg_layout_writer import write_jpeg3
    S = args.size
    pre = DevicePreprocessor(S, "cuda:0")
    kw = dict(non_rgb="convert", cmyk="device", layouts="all")
    cmyk = []
    for k in range(4):
        buf = io.BytesIO()
        Image.fromarray(synthetic_rgb(4608, 3456, seed=k)).convert("CMYK").save(buf, format="JPEG", quality=90,
                                                                               subsampling=2)
        cmyk.append(buf.getvalue())
    two = [write_jpeg3(picture(1536, 2048, seed=k, noise=True), *LAYOUTS["440"], q=12) for k in range(2)]
    cases = [("cmyk 4:2:0-style (component 0 at 2x2)", "device-cmyk", (3456, 4608), cmyk),
             ("4:4:0", "device-layout", (2048, 1536), [two[k % 2] for k in range(4)])]
    lines = []
    for name, route, (w, h), blobs in cases:
        fns = {"decode": lambda dl: pre.decode_jpeg(blobs, draft=(S, S), draft_layouts=dl, **kw),
               "decode_resize": lambda dl: pre.from_jpeg_bytes(blobs, draft=True, draft_layouts=dl, **kw)}
        dev = fns["decode"]("all")
        assert pre.last_routes == (route,) * len(blobs), pre.last_routes
        host = fns["decode"]("common")
        assert pre.last_routes == ("host",) * len(blobs), pre.last_routes
        assert all(torch.equal(a, b) for a, b in zip(dev, host)), "the device's drafted pixels differ from Pillow's"
        scale = J.draft_scale((w, h), (S, S))
        line = {"kind": name, "route": route, "width": w, "height": h, "batch": len(blobs), "draft_scale": scale,
                "drafted_size": list(J.scaled_size((w, h), scale)),
                "mean_jpeg_bytes": int(np.mean([len(b) for b in blobs])), "iters": args.iters,
                "gpu": torch.cuda.get_device_name(0)}
        for fname, fn in fns.items():
            for _ in range(args.warmup):
                fn("common")
                fn("all")
            torch.cuda.synchronize()
            t = {"common": [], "all": []}
            for _ in range(args.iters):
                for dl in ("common", "all"):
                    t0 = time.perf_counter()
                    fn(dl)
                    torch.cuda.synchronize()
                    t[dl].append(1e3 * (time.perf_counter() - t0))
            for dl in ("common", "all"):
                q1, med, q3 = (float(x) for x in np.percentile(t[dl], [25, 50, 75]))
                line[f"{fname}_{dl}_ms"] = {"median": med, "q1": q1, "q3": q3, "min": float(min(t[dl]))}
            line[f"{fname}_common_over_all"] = line[f"{fname}_common_ms"]["median"] / line[f"{fname}_all_ms"]["median"]
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out and lines:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def with_orientation(blob: bytes, orientation: int) -> bytes:
    """The file with an Exif APP1 that holds the Orientation tag alone, behind its JFIF APP0."""
    from PIL import Image
    exif = Image.Exif()
    exif[0x0112] = orientation
    payload = exif.tobytes()
    pos = 2
    if blob[2:4] == b"\xff\xe0":
        pos = 4 + int.from_bytes(blob[4:6], "big")
    return blob[:pos] + b"\xff\xe1" + (len(payload) + 2).to_bytes(2, "big") + payload + blob[pos:]


def _quartiles(ts):
    q1, med, q3 = (float(x) for x in np.percentile(ts, [25, 50, 75]))
    return {"median": med, "q1": q1, "q3": q3, "min": float(min(ts))}


def orient_bench(args):
    """The orient launch against a device-to-device copy, then orientation="exif" end to end."""
    import tempfile
    import torch
    from on_device_image_captioning_amd import _hip
    from on_device_image_captioning_amd.image_utils import ORIENT_JOB_DTYPE, DevicePreprocessor
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    lib = _hip.load()
    lines = []

    def event_us(fn, reps):
        """Median / quartiles / min of the time per call over args.iters windows of `reps` calls each."""
        for _ in range(args.warmup * reps):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ts.append(1e3 * a.elapsed_time(b) / reps)
        return _quartiles(ts)

    for (W, H), n, reps in (((4032, 3024), 1, 50), ((640, 480), 1, 500), ((640, 480), 16, 200)):
        nbytes = 3 * W * H
        slot = (nbytes + 255) // 256 * 256
        src = torch.randint(0, 256, (n * slot,), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        stream = torch.cuda.current_stream().cuda_stream
        line = {"kernel": "odic_orient_rgb8", "width": W, "height": H, "images": n, "bytes_each_way": n * nbytes,
                "launches_per_window": reps, "iters": args.iters, "gpu": torch.cuda.get_device_name(0)}
        copy = event_us(lambda: dst.copy_(src), reps)
        line["copy_us"] = copy
        for o in range(2, 9):
            rec = np.zeros(n, ORIENT_JOB_DTYPE)
            rec["src_off"] = rec["dst_off"] = np.arange(n) * slot
            rec["src_stride_bytes"], rec["H"], rec["W"], rec["orientation"] = 3 * W, H, W, o
            t = event_us(lambda: _hip.check(lib.odic_orient_rgb8(rec.ctypes.data, n, src.data_ptr(), dst.data_ptr(),
                                                                 stream), "odic_orient_rgb8"), reps)
            line[f"orient_{o}_us"] = t
            line[f"orient_{o}_over_copy"] = t["median"] / copy["median"]
            line[f"orient_{o}_GBps"] = 2 * n * nbytes / t["median"] / 1e3
        line["copy_GBps"] = 2 * n * nbytes / copy["median"] / 1e3
        line["copy_again_us"] = event_us(lambda: dst.copy_(src), reps)       # the spread of the yardstick itself
        print(json.dumps(line), flush=True)
        lines.append(line)

    pre = DevicePreprocessor(args.size, "cuda:0")
    B = 16
    blobs = [with_orientation(b, 6) for b in make_inputs(B)]
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for k, b in enumerate(blobs):
            paths.append(os.path.join(d, f"{k}.jpg"))
            with open(paths[-1], "wb") as f:
                f.write(b)
        fns = {"host_exif": lambda: pre.from_files(paths, decode="host", orientation="exif"),
               "device_exif": lambda: pre.from_jpeg_bytes(blobs, orientation="exif"),
               "device_ignore": lambda: pre.from_jpeg_bytes(blobs)}
        assert torch.equal(fns["host_exif"](), fns["device_exif"]()), "host and device paths differ"
        assert pre.last_routes == ("device",) * B and pre.last_orientations == (6,) * B
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.iters):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                t[name].append(1e3 * (time.perf_counter() - t0))
    line = {"end_to_end": "16 files 640x480 q90 4:2:0, orientation 6", "iters": args.iters, "size": args.size,
            "gpu": torch.cuda.get_device_name(0)}
    for k, v in t.items():
        line[f"{k}_ms"] = _quartiles(v)
    line["host_over_device_exif"] = line["host_exif_ms"]["median"] / line["device_exif_ms"]["median"]
    line["exif_minus_ignore_ms"] = _quartiles([a - b for a, b in zip(t["device_exif"], t["device_ignore"])])
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="also time the device path at other subseq_bits / passes")
    ap.add_argument("--progressive", action="store_true", help="progressive re-saves of the crops, and tatin.jpg")
    ap.add_argument("--gray", action="store_true", help="the crops as one-component files, non_rgb='convert'")
    ap.add_argument("--cmyk", action="store_true", help="the crops as four-component files, non_rgb='convert', cmyk='device'")
    ap.add_argument("--layouts", action="store_true", help="4:4:0 and 4:1:1 files from the tests' writer, layouts='all'")
    ap.add_argument("--progressive-layouts", action="store_true",
                    help="progressive 4:4:0 from the tests' writer and Pillow's progressive CMYK, every opt-in")
    ap.add_argument("--draft", action="store_true", help="draft off against draft on, large and small synthetic files")
    ap.add_argument("--draft-cases", choices=["all", "large"], default="all")
    ap.add_argument("--draft-layouts", action="store_true",
                    help="large CMYK and 4:4:0 files under a draft, draft_layouts='common' against 'all'")
    ap.add_argument("--orient", action="store_true", help="odic_orient_rgb8 against a copy; orientation='exif' end to end")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.draft:
        return draft_bench(args)
    if args.draft_layouts:
        return draft_layouts_bench(args)
    if args.orient:
        return orient_bench(args)

    import torch
    from PIL import Image
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    assert torch.cuda.is_available(), "jpeg_bench needs a GPU"
    pre = DevicePreprocessor(args.size, "cuda:0")
    if args.cmyk and (args.gray or args.progressive):
        ap.error("--cmyk goes alone: the four-component route is baseline only")
    if args.layouts and (args.gray or args.progressive or args.cmyk):
        ap.error("--layouts goes alone: the route is baseline three-component files only")
    both = args.progressive_layouts
    if both and (args.gray or args.progressive or args.cmyk or args.layouts):
        ap.error("--progressive-layouts goes alone: it sets every opt-in itself")
    non_rgb = "convert" if args.gray or args.cmyk or both else "black"
    route_kw = {"cmyk": "device"} if args.cmyk else {"layouts": "all"} if args.layouts else {}
    want_route = ("device-cmyk" if args.cmyk else "device-layout" if args.layouts else
                  "device-progressive" if args.progressive else "device")
    names = {}                                           # id of a batch's list → its layout
    if both:
        route_kw = {"cmyk": "device", "layouts": "all"}
        inputs = []
        for kind, blobs_all in (("440", progressive_layout_inputs("440", max(args.batches))),
                                ("cmyk", make_inputs(max(args.batches), progressive=True, cmyk=True))):
            for B in args.batches:
                inputs.append((B, blobs_all[:B], (640, 480)))
                names[id(inputs[-1][1])] = kind
    elif args.layouts:
        inputs = []
        for layout in ("440", "411"):
            blobs_all = layout_inputs(layout, max(args.batches))
            for B in args.batches:
                inputs.append((B, blobs_all[:B], (640, 480)))
                names[id(inputs[-1][1])] = layout
    else:
        blobs_all = make_inputs(max(args.batches), progressive=args.progressive, gray=args.gray, cmyk=args.cmyk)
        inputs = [(B, blobs_all[:B], (640, 480)) for B in args.batches]
    parse_us = None
    if args.progressive:
        from on_device_image_captioning_amd import jpeg as J
        with open(os.path.join(ROOT, "tests", "golden", "demo_material", "tatin.jpg"), "rb") as f:
            tatin = f.read()
        if not args.gray:                                # tatin.jpg is a colour file
            inputs += [(1, [tatin], (1280, 960)), (16, [tatin] * 16, (1280, 960))]
        t0 = time.perf_counter()
        for _ in range(5):
            for b in blobs_all:
                J.parse(b, non_rgb)
                J.parse_progressive(b, non_rgb)
        parse_us = 1e6 * (time.perf_counter() - t0) / (5 * len(blobs_all))

    def host(blobs):
        if args.gray or args.cmyk or args.layouts or both:
            return pre([np.asarray(Image.open(io.BytesIO(b)).convert("RGB")) for b in blobs])
        return pre([np.asarray(Image.open(io.BytesIO(b))) for b in blobs])

    def device(blobs):
        return pre.from_jpeg_bytes(blobs, progressive="device" if args.progressive or both else "host", non_rgb=non_rgb,
                                   **route_kw)

    lines = []
    for B, blobs, (width, height) in inputs:
        if args.device_only:
            for _ in range(args.warmup + args.iters):
                device(blobs)
            torch.cuda.synchronize()
            continue
        assert torch.equal(host(blobs), device(blobs)), "host and device paths differ"
        if both:
            want_route = {"440": "device-progressive-layout", "cmyk": "device-progressive-cmyk"}[names[id(blobs)]]
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
                    fn = lambda b, bits=bits, passes=passes: pre.from_jpeg_bytes(   # noqa: E731
                        b, bits, passes, non_rgb=non_rgb, **route_kw)
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
        line = {"batch": B, "width": width, "height": height, "quality": 90,
                "subsampling": "gray" if args.gray else "cmyk 2x2,1x1,1x1,1x1" if args.cmyk else
                {"440": "4:4:0", "411": "4:1:1", "cmyk": "cmyk 2x2,1x1,1x1,1x1"}[names[id(blobs)]]
                if args.layouts or both else "4:2:0",
                "progressive": args.progressive or both,
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
