"""Draft-scale decode of CMYK / YCCK and any-layout JPEGs on the device: `decode_jpeg(..., draft=, draft_layouts="all")`
against the host route and against Pillow's drafted `convert("RGB")` bit for bit — a mixed batch that holds scales 1, 2, 4
and 8 at once, the full case list of jpeg_draft_layout_model (baseline and progressive, with and without restart
intervals), regions and EXIF orientation on the drafted image, the two _scaled entry points' treatment of a null or
invalid scale, and the default's routes."""
import ctypes
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_draft_layout_model as M
from guards import guarded
from jpeg_exif_cases import with_orientation
from jpeg_gray_cases import png
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

ON = dict(progressive="device", non_rgb="convert", cmyk="device", layouts="all")
ALL = dict(draft_layouts="all", **ON)
OWN = ("device-cmyk", "device-layout", "device-progressive-cmyk", "device-progressive-layout")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


def drafted(blob, req):
    im = Image.open(io.BytesIO(blob))
    if im.format == "JPEG":
        im.draft("RGB", req)
    return torch.from_numpy(np.asarray(im.convert("RGB"), dtype=np.uint8).copy())


def mixed():
    """[(bytes, route under draft_layouts="all", scale under the request (12, 12))]"""
    return [(encode(smooth_rgb(17, 13, seed=1), quality=90, subsampling=2), "device", 1),
            (encode(smooth_rgb(41, 30, seed=2), quality=90, subsampling=1, progressive=True), "device-progressive", 2),
            (M.Case("photoshop-ycck", 97, 101, seed=3).baseline(), "device-cmyk", 8),
            (M.Case("440", 50, 61, seed=4, restart=2).baseline(), "device-layout", 4),
            (png("RGBA", 19, 23), "host", 1),
            (M.Case("cmyk-21", 30, 41, seed=5).progressive(), "device-progressive-cmyk", 2),
            (M.Case("410", 99, 120, seed=6).progressive(), "device-progressive-layout", 8),
            (M.Case("22-12-12", 23, 19, seed=7).baseline(), "device-layout", 1),
            (M.Case("ycck-22", 50, 50, seed=8).split_refine(), "device-progressive-cmyk", 4)]


def test_mixed_batch_with_every_scale_at_once(pre):
    files = mixed()
    blobs, routes = [f for f, _, _ in files], [r for _, r, _ in files]
    req = (12, 12)
    hdr_sizes = [Image.open(io.BytesIO(b)).size for b in blobs]
    assert [J.draft_scale(s, req) for s in hdr_sizes] == [s for _, _, s in files]
    assert {s for _, r, s in files if r in OWN} == {1, 2, 4, 8}
    got = pre.decode_jpeg(blobs, draft=req, **ALL)
    assert list(pre.last_routes) == routes and set(OWN) <= set(routes)
    host = pre.decode_jpeg(blobs, draft=req, draft_layouts="common", **ON)
    assert list(pre.last_routes) == [r if r not in OWN else "host" for r in routes]
    for k, (g, h, b) in enumerate(zip(got, host, blobs)):
        assert torch.equal(g, h) and torch.equal(g.cpu(), drafted(b, req)), k


def test_the_default_sends_them_to_the_host(pre):
    files = mixed()
    blobs, routes = [f for f, _, _ in files], [r for _, r, _ in files]
    got = pre.decode_jpeg(blobs, draft=(12, 12), **ON)
    assert list(pre.last_routes) == [r if r not in OWN else "host" for r in routes]
    for g, b in zip(got, blobs):
        assert torch.equal(g.cpu(), drafted(b, (12, 12)))
    with pytest.raises(ValueError, match="draft_layouts must be 'common' or 'all'"):
        pre.decode_jpeg(blobs, draft=(12, 12), draft_layouts="every", **ON)
    with pytest.raises(ValueError, match="draft_layouts"):
        pre.from_jpeg_bytes(blobs, draft_layouts="device")


@pytest.fixture(scope="module")
def case_files():
    """name → [(kind, bytes)]: baseline, progressive under the standard script, progressive with split refinements.  The
    48 x 64 cases carry restart intervals in the first two."""
    return {n: [("baseline", c.baseline()), ("progressive", c.progressive()), ("split-refine", c.split_refine())]
            for n, c in M.CASES.items()}


@pytest.mark.parametrize("scale", M.SCALES)
def test_every_case_file(pre, case_files, scale):
    done = 0
    for size in M.SIZES:
        req = M.request_for(size, scale)
        if J.draft_scale(size, req) != scale:             # an image 3 pixels across cannot be asked for 1/4
            continue
        names = [n for n, c in M.CASES.items() if c.size == size]
        assert len(names) == len(M.LAYOUTS)
        labels = [(n, kind) for n in names for kind, _ in case_files[n]]
        blobs = [b for n in names for _, b in case_files[n]]
        got = pre.decode_jpeg(blobs, draft=req, **ALL)
        want_routes = [("device-progressive-" if kind != "baseline" else "device-") +
                       ("cmyk" if M.CASES[n].ncomp == 4 else "layout") for n, kind in labels]
        assert list(pre.last_routes) == want_routes, size   # none on the host, none "host-after-status"
        wrong = []
        for label, g, b in zip(labels, got, blobs):
            want = drafted(b, req)
            if g.shape != want.shape or not torch.equal(g.cpu(), want):
                wrong.append(label)
        assert not wrong, (size, wrong)
        done += len(blobs)
    assert done >= 3 * 3 * len(M.LAYOUTS)
    if scale == 2:
        assert any(c.restart for c in M.CASES.values())


def test_regions_and_orientation_on_the_drafted_image():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    small = DevicePreprocessor(32, "cuda:0", max_pixels=256 * 256)            # draft=True requests (32, 32): scale 2
    blobs = [with_orientation(M.CASES["photoshop-ycck-93x67"].baseline(), 6),
             with_orientation(M.CASES["440-93x67"].baseline(), 3),
             M.CASES["440-93x67"].progressive()]
    assert J.draft_scale((93, 67), (32, 32)) == 2 and J.scaled_size((93, 67), 2) == (47, 34)
    kw = dict(draft=True, orientation="exif")
    whole = small.from_jpeg_bytes(blobs, **kw, **ALL)
    assert small.last_routes == ("device-cmyk", "device-layout", "device-progressive-layout")
    assert small.last_orientations == (6, 3, 1)
    assert torch.equal(whole, small.from_jpeg_bytes(blobs, **kw, **ON))
    assert small.last_routes == ("host", "host", "host")
    # boxes in the drafted, upright coordinates: image 0 is 34 x 47 after the turn
    regions = [(0, (1.5, 2.0, 30.0, 44.25)), (1, (0.0, 1.0, 47.0, 33.5)), (2, (10.25, 3.0, 40.0, 20.0)),
               (0, (0.0, 0.0, 34.0, 47.0))]
    a = small.from_jpeg_bytes(blobs, regions=regions, **kw, **ALL)
    assert small.last_routes == ("device-cmyk", "device-layout", "device-progressive-layout")
    b = small.from_jpeg_bytes(blobs, regions=regions, **kw, **ON)
    assert a.shape == (4, 3, 32, 32) and torch.equal(a, b)
    with pytest.raises(ValueError):
        small.from_jpeg_bytes(blobs, regions=[(0, (0.0, 0.0, 47.0, 34.0))], **kw, **ALL)      # the undrafted turn's box


SCALED_ENTRIES = {"device-cmyk": ("photoshop-ycck-93x67", "baseline"), "device-layout": ("410-93x67", "baseline"),
                  "device-progressive-layout": ("22-21-21-93x67", "progressive"),
                  "device-progressive-cmyk": ("cmyk-21-93x67", "progressive")}


@pytest.mark.parametrize("route", SCALED_ENTRIES)
def test_scaled_decodes_stay_inside_their_buffers(route, monkeypatch):
    """One file through its _scaled entry point with the workspace, the compressed-data copy, the RGB output and `status`
    each exactly as large as asked for inside a poisoned allocation.  At a valid scale nothing outside them is written;
    with scale_log2 = 4 the status is 1 and nothing of the output is written either."""
    from on_device_image_captioning_amd import image_utils
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    made = []
    orig = DevicePreprocessor._grow

    def exact(buf, nbytes, **kw):
        if "device" not in kw:
            return orig(buf, nbytes, **kw)
        g = guarded(1, max(nbytes, 1), max(nbytes, 1), torch.uint8, kw["device"])
        made.append(g)
        return g.t.view(-1)

    class TorchWithGuardedEmpty:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*size, **kw):
            if kw.get("device") is not None and not kw.get("pin_memory") and len(size) == 1 and isinstance(size[0], int) \
                    and kw.get("dtype") in (torch.uint8, torch.int32) and torch.device(kw["device"]).type == "cuda":
                g = guarded(1, size[0], size[0], kw["dtype"], kw["device"])
                made.append(g)
                return g.t.view(-1)
            return torch.empty(*size, **kw)

    monkeypatch.setattr(DevicePreprocessor, "_grow", staticmethod(exact))
    fresh = DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)
    monkeypatch.setattr(image_utils, "torch", TorchWithGuardedEmpty())
    name, kind = SCALED_ENTRIES[route]
    case = M.CASES[name]
    blob = case.baseline() if kind == "baseline" else case.progressive()
    called = []
    real_check = fresh._hip.check
    monkeypatch.setattr(fresh._hip, "check", lambda code, what: (called.append(what), real_check(code, what))[1])
    for scale in (2, 8):
        req = M.request_for(case.size, scale)
        w, h = J.scaled_size(case.size, scale)
        got, = fresh.decode_jpeg([blob], draft=req, **ALL)
        torch.cuda.synchronize()
        assert fresh.last_routes == (route,) and called[-1].endswith("_scaled")
        assert torch.equal(got.cpu(), drafted(blob, req))
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        for g in made:
            g.assert_untouched(what=f"{route} at 1/{scale}, {g.dtype} buffer of {g.cols} elements")
        assert len([g for g in made if g.dtype == torch.uint8 and g.cols == w * h * 3]) == 1
        made.clear()

    # a scale that is none: the plan's scale_log2 section is overwritten with 4 on its way to the device
    real_plan = J.plan_device_batch

    def plan_with_scale_4(*a, **kw):
        p = real_plan(*a, **kw)
        for o, arr in p.sections:
            if o == p.scale_off:
                arr[:] = 4
        return p

    monkeypatch.setattr(J, "plan_device_batch", plan_with_scale_4)
    req = M.request_for(case.size, 2)
    w, h = J.scaled_size(case.size, 2)
    got, = fresh.decode_jpeg([blob], draft=req, **ALL)
    torch.cuda.synchronize()
    assert fresh.last_routes == ("host-after-status",) and called[-1].endswith("_scaled")
    assert torch.equal(got.cpu(), drafted(blob, req))          # PIL's, after the device said 1
    for g in made:
        g.assert_untouched(what=f"{route} with scale_log2 = 4, {g.dtype} buffer of {g.cols} elements")
    out, = [g for g in made if g.dtype == torch.uint8 and g.cols == w * h * 3]
    assert bool((out.t == 0xFF).all()), "an image with an invalid scale has none of its pixels written"


def test_a_null_scale_array_is_refused(pre):
    lib, hip = pre.lib, pre._hip
    b = hip.JpegBatch()
    b.headers, b.data, b.out, b.status = 16, 16, 16, 16
    b.n_images, b.subseq_bits, b.max_sync_passes = 1, 512, 4
    b.max_units = b.max_intervals = b.max_width = b.max_height = 1
    b.max_blocks = b.max_scan_bytes = b.total_scan_bytes = b.total_intervals = b.total_units = 1
    b.total_blocks = b.total_plane_bytes = 1
    need = lib.odic_jpeg_any_workspace_bytes(ctypes.byref(b))
    assert need > 0 and lib.odic_jpeg_any_decode_scaled(ctypes.byref(b), None, 16, need, None) == -2
    p = hip.JpegProgBatch()
    p.headers = p.scans = p.tables = p.data = p.out = p.status = 16
    assert lib.odic_jpeg_decode_progressive_any_scaled(ctypes.byref(p), None, 16, 1 << 20, None) == -2
