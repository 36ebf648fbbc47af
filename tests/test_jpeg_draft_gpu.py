"""Scaled (draft) JPEG decode on the GPU (odic_jpeg_decode_scaled / odic_jpeg_decode_progressive_scaled through
DevicePreprocessor.decode_jpeg(draft=) / from_jpeg_bytes / from_files(draft=True)) against Pillow's `Image.draft`, bit
for bit."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

import guards
import test_jpeg_host as H
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_draft_host import model_coefficients, model_draft_rgb, noise_rgb, pil_draft, request_for
from test_jpeg_host import encode, smooth_rgb
from test_jpeg_progressive_host import encode_progressive

pytestmark = pytest.mark.gpu

SIZES = [(75, 101), (17, 33), (8, 8), (1, 1)]             # (w, h)
QUALITIES = (30, 90, 100)
KINDS = ("baseline", "dri", "progressive")
DEVICE_ROUTES = {"baseline": "device", "dri": "device", "progressive": "device-progressive"}


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0")


def gradient_rgb(h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)],
                    axis=2).astype(np.uint8)


def save(img, kind, **kw):
    if kind == "progressive":
        return encode_progressive(img, **kw)
    return encode(img, **(dict(kw, restart_marker_blocks=2) if kind == "dri" else kw))


@functools.lru_cache(maxsize=None)
def matrix_files(sampling, size):
    """[(kind, blob, the baseline twin's parsed coefficients)] for one sampling and size: noise at three qualities, and
    a smooth gradient for the largest size.  A kind changes the entropy coding only, never the coefficients."""
    w, h = size
    images = [(noise_rgb(h, w, seed=q + w), q) for q in QUALITIES]
    if size == SIZES[0]:
        images.append((gradient_rgb(h, w), 90))
    out = []
    for img, q in images:
        parsed = model_coefficients(save(img, "baseline", quality=q, subsampling=sampling))
        out += [(kind, save(img, kind, quality=q, subsampling=sampling), parsed) for kind in KINDS]
    return out


def decode_and_compare(pre, blobs, req, **kw):
    """decode_jpeg with a draft request against the host sequence, file by file → (routes, scales Pillow chose)."""
    got = pre.decode_jpeg(blobs, draft=req, **kw)
    routes, scales = pre.last_routes, []
    assert len(got) == len(blobs)
    for k, (g, b) in enumerate(zip(got, blobs)):
        want, s = pil_draft(b, req)
        scales.append(s)
        g = g.cpu().numpy()
        assert g.shape == want.shape, (k, g.shape, want.shape)
        assert np.array_equal(g, want), (k, routes[k], s, int(np.abs(g.astype(int) - want).max()))
    return routes, scales


@pytest.mark.parametrize("sampling", [0, 1, 2], ids=["444", "422", "420"])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_exactness_matrix(pre, s, sampling):
    for size in SIZES:
        files = matrix_files(sampling, size)
        req = request_for(size, s)
        routes, scales = decode_and_compare(pre, [f[1] for f in files], req, progressive="device")
        want_scale = s if min(size) >= s else 1                                   # 1 x 1 cannot be drafted
        assert scales == [want_scale] * len(files)
        for (kind, _, parsed), route in zip(files, routes):
            # on the CPU: the file's dequantised inputs, pass-1 values and results stay inside the device's limits,
            # so an exact result cannot come from the host fallback
            if want_scale > 1:
                model_draft_rgb(None, want_scale, parsed)                         # raises H.Rejected outside them
            assert route == DEVICE_ROUTES[kind], (size, kind, route)      # every file, not just nine in ten


def test_mixed_scales_in_one_call(pre):
    """One request, image sizes that draft at 1, 2, 4 and 8, baseline and progressive in the same call."""
    req = (16, 16)
    sizes = [(20, 24), (40, 33), (70, 77), (130, 129), (31, 200), (129, 140)]
    blobs = []
    for k, (w, h) in enumerate(sizes):
        img = smooth_rgb(h, w, seed=k)
        blobs.append(encode(img, quality=90, subsampling=k % 3))
        blobs.append(encode_progressive(img, quality=85, subsampling=(k + 1) % 3))
    routes, scales = decode_and_compare(pre, blobs, req, progressive="device")
    assert scales == [1, 1, 2, 2, 4, 4, 8, 8, 1, 1, 8, 8]
    assert routes == ("device", "device-progressive") * len(sizes)
    drafted = [t.cpu() for t in pre.decode_jpeg(blobs, draft=req, progressive="device")]
    plain = [t.cpu() for t in pre.decode_jpeg(blobs, progressive="device")]
    for k, s in enumerate(scales):
        assert torch.equal(drafted[k], plain[k]) == (s == 1), k
    # without progressive="device" the progressive files take the host route, with the same request
    routes, _ = decode_and_compare(pre, blobs, req)
    assert routes == ("device", "host") * len(sizes)


def stress_files():
    cb = ((np.indices((40, 40)).sum(0) % 2) * 255).astype(np.uint8)
    swing = (np.random.default_rng(2).integers(0, 2, (40, 40, 3)) * 255).astype(np.uint8)
    noise = noise_rgb(40, 40, seed=9)
    coarse = [[255] * 64, [255] * 64]
    out = []
    for sampling in (0, 1, 2):
        out.append(encode(np.stack([cb, 255 - cb, cb], 2), quality=100, subsampling=sampling))
        out.append(encode(swing, quality=100, subsampling=sampling))
        out.append(encode(swing, qtables=coarse, subsampling=sampling))
        out.append(encode_progressive(swing, qtables=coarse, subsampling=sampling))
        # quality-100 noise under flat tables: dequantised inputs and pass-1 values on both sides of ±8191
        out += [H.flat_dqt(encode(noise, quality=100, subsampling=sampling), v) for v in (6, 12, 255)]
    return out


@pytest.mark.parametrize("s", [2, 4, 8])
def test_inputs_that_stress_the_range_limits(pre, s):
    blobs = stress_files()
    routes, scales = decode_and_compare(pre, blobs, request_for((40, 40), s), progressive="device")
    assert scales == [s] * len(blobs)
    seen = set()
    for blob, route in zip(blobs, routes):
        assert route in ("device", "device-progressive", "host-after-status"), route
        if J.parse(blob).kind == J.DEVICE:                # baseline: the model says which route it has to be
            try:
                model_draft_rgb(blob, s)
                assert route == "device"
            except H.Rejected:
                assert route == "host-after-status"       # a pass: the host decoded it again with the same request
        seen.add(route)
    assert {"device", "host-after-status"} <= seen


def test_scaled_decode_stays_inside_its_buffers(monkeypatch):
    """As test_jpeg_progressive_decode_stays_inside_its_workspace, for both _scaled entry points: the workspace, the
    data copy, the RGB output (now the scaled images' bytes) and `status` are exactly the requested bytes inside
    poisoned allocations; the uploaded data, records and scales are unchanged afterwards."""
    from on_device_image_captioning_amd import image_utils
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    made = []
    orig = DevicePreprocessor._grow

    def exact(buf, nbytes, **kw):
        if "device" not in kw:
            return orig(buf, nbytes, **kw)
        g = guards.guarded(1, max(nbytes, 1), max(nbytes, 1), torch.uint8, kw["device"])
        made.append(g)
        return g.t.view(-1)

    class TorchWithGuardedEmpty:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*size, **kw):
            if kw.get("device") is not None and not kw.get("pin_memory") and len(size) == 1 and isinstance(size[0], int) \
                    and kw.get("dtype") in (torch.uint8, torch.int32) and torch.device(kw["device"]).type == "cuda":
                g = guards.guarded(1, size[0], size[0], kw["dtype"], kw["device"])
                made.append(g)
                return g.t.view(-1)
            return torch.empty(*size, **kw)

    monkeypatch.setattr(DevicePreprocessor, "_grow", staticmethod(exact))
    pre = DevicePreprocessor(384, "cuda:0")
    monkeypatch.setattr(image_utils, "torch", TorchWithGuardedEmpty())
    base = [encode(smooth_rgb(h, w, seed=k), quality=90, subsampling=k % 3)
            for k, (w, h) in enumerate([(75, 101), (17, 33), (130, 129)])]
    prog = [encode_progressive(smooth_rgb(h, w, seed=k), quality=90, subsampling=k % 3)
            for k, (w, h) in enumerate([(33, 70), (129, 140), (8, 8)])]
    kinds = set()
    for batch, req in ((base + prog, (16, 16)), (base, (9, 12)), (prog, (4, 8)), (base[:1], (75, 101)),
                       (prog + base, (1, 1))):
        routes, scales = decode_and_compare(pre, batch, req, progressive="device")
        assert set(routes) <= {"device", "device-progressive"}
        torch.cuda.synchronize()
        dev, pinned = pre._jpeg_dev, pre._jpeg_pinned
        n = min(dev.numel(), pinned.numel())
        assert n >= sum(len(b) for b in batch) and torch.equal(dev[:n].cpu(), pinned[:n]), "inputs are only read"
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        out_bytes = sum(w * h * 3 for w, h in (J.scaled_size(Image.open(io.BytesIO(b)).size, s)
                                               for b, s in zip(batch, scales)))
        assert any(g.dtype == torch.uint8 and g.cols == out_bytes for g in made), "the output holds the scaled images only"
        assert any(g.dtype == torch.int32 and g.cols == len(batch) for g in made)
        for g in made:
            g.assert_untouched(what=f"scaled jpeg decode, {g.dtype} buffer of {g.cols} elements")
            kinds.add(g.dtype)
        made.clear()
    assert kinds == {torch.uint8, torch.int32}


def test_from_files_draft_device_equals_host(pre, tmp_path):
    paths = []
    for k, (w, h) in enumerate([(400, 300), (1600, 1200), (500, 400)]):
        p = tmp_path / f"f{k}.jpg"
        p.write_bytes(encode(smooth_rgb(h, w, seed=k), quality=90, subsampling=2))
        paths.append(str(p))
    assert [J.draft_scale(s, (384, 384)) for s in ((400, 300), (1600, 1200), (500, 400))] == [1, 2, 1]
    dev = pre.from_files(paths, decode="device", draft=True)
    assert pre.last_routes == ("device",) * 3
    host = pre.from_files(paths, decode="host", draft=True)
    assert torch.equal(dev, host)
    plain = pre.from_files(paths, decode="device")
    assert torch.equal(plain, pre.from_files(paths))
    assert torch.equal(dev[0], plain[0]) and torch.equal(dev[2], plain[2])          # scale 1: today's path
    assert not torch.equal(dev[1], plain[1])                                        # scale 2: really engaged
    with open(paths[1], "rb") as f:
        assert tuple(pre.decode_jpeg([f.read()], draft=(384, 384))[0].shape) == (600, 800, 3)


def test_black_canvases_have_the_drafted_size(pre):
    g = io.BytesIO()
    Image.fromarray(smooth_rgb(30, 40)[:, :, 0]).save(g, format="JPEG")
    c = io.BytesIO()
    Image.fromarray(smooth_rgb(33, 41)).convert("CMYK").save(c, format="JPEG")
    blobs = [g.getvalue(), c.getvalue()]
    routes, scales = decode_and_compare(pre, blobs, (5, 5), progressive="device")
    assert routes == ("black", "black") and scales == [4, 4]
    got = pre.decode_jpeg(blobs, draft=(5, 5))
    assert [tuple(t.shape) for t in got] == [(8, 10, 3), (9, 11, 3)] and all(int(t.max()) == 0 for t in got)
    assert [tuple(t.shape) for t in pre.decode_jpeg(blobs)] == [(30, 40, 3), (33, 41, 3)]
    with pytest.raises(ValueError):
        pre.decode_jpeg(blobs, draft=(0, 5))
