"""Three-component JPEGs at every baseline sampling layout on the device: `decode_jpeg(..., layouts="all")` against
`np.asarray(Image.open(f).convert("RGB"))` bit for bit under four knob settings, a mixed batch with every other kind, the
default's routes, a draft request, EXIF orientation, and the containment of odic_jpeg3_any_decode."""
import io
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import jpeg_cmyk_cases as K
import jpeg_layout_cases as L
from guards import guarded
from jpeg_exif_cases import with_orientation
from jpeg_gray_cases import gray_file
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

KNOBS = {"default": dict(), "subseq32": dict(subseq_bits=32), "serial": dict(max_sync_passes=0),
         "subseq32-serial": dict(subseq_bits=32, max_sync_passes=0)}
ALL = dict(layouts="all")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


@pytest.fixture(scope="module")
def oracles():
    return {name: torch.from_numpy(L.oracle(c.blob).copy()) for name, c in L.CASES.items()}


@pytest.mark.parametrize("knobs", KNOBS)
def test_every_case_file(pre, oracles, knobs):
    names = list(L.CASES)
    got = pre.decode_jpeg([L.CASES[n].blob for n in names], **ALL, **KNOBS[knobs])
    routes = dict(zip(names, pre.last_routes))
    assert routes == {n: "device-layout" for n in names}         # none on the host, none "host-after-status"
    wrong = [n for n, g in zip(names, got) if g.shape != oracles[n].shape or not torch.equal(g.cpu(), oracles[n])]
    assert not wrong, wrong
    for n in names[::11]:                                        # ... and alone
        g, = pre.decode_jpeg([L.CASES[n].blob], **ALL, **KNOBS[knobs])
        assert pre.last_routes == ("device-layout",) and torch.equal(g.cpu(), oracles[n]), n


def mixed():
    files = [(encode(smooth_rgb(48, 64, seed=1), quality=90, subsampling=2), "device", "device"),
             (encode(smooth_rgb(40, 56, seed=2), quality=90, subsampling=1, progressive=True), "device-progressive",
              "device-progressive"),
             (gray_file("dri3", (37, 53)), "device", "device"),
             (K.CASES["cmyk-sub2-48x64"][0], "device-cmyk", "device-cmyk"),
             (L.CASES["440-17x33"].blob, "device-layout", "host"),
             (L.CASES["411-dri3"].blob, "device-layout", "host"),
             (L.CASES["410-48x64"].blob, "device-layout", "host"),
             (L.CASES["rgb-22-17x33"].blob, "device-layout", "host"),
             (L.CASES["11-21-21-7x9"].blob, "device-layout", "host")]
    random.Random(7).shuffle(files)
    return [f for f, _, _ in files], [r for _, r, _ in files], [r for _, _, r in files]


def test_mixed_batch_and_the_default(pre):
    blobs, routes, default_routes = mixed()
    want = [torch.from_numpy(L.oracle(b).copy()) for b in blobs]
    kw = dict(non_rgb="convert", cmyk="device", progressive="device")
    got = pre.decode_jpeg(blobs, **kw, **ALL)
    assert list(pre.last_routes) == routes
    plain = pre.decode_jpeg(blobs, **kw)                         # without the keyword: the same pixels, by PIL
    assert list(pre.last_routes) == default_routes
    for k, (g, h, w) in enumerate(zip(got, plain, want)):
        assert torch.equal(g.cpu(), w) and torch.equal(g, h), k
    assert torch.equal(pre.from_jpeg_bytes(blobs, **kw, **ALL), pre.from_jpeg_bytes(blobs, **kw))
    regions = [(routes.index("device-layout"), (1.5, 2.0, 6.0, 8.25)), (0, (0.0, 1.0, 7.0, 8.5))]
    assert torch.equal(pre.from_jpeg_bytes(blobs, regions=regions, **kw, **ALL),
                       pre.from_jpeg_bytes(blobs, regions=regions, **kw))
    with pytest.raises(ValueError, match="layouts"):
        pre.decode_jpeg(blobs, layouts="every")


def test_draft_request_and_refused_files_stay_on_the_host(pre):
    blobs = [L.CASES["440-48x64"].blob, L.CASES["411-48x64"].blob]
    got = pre.decode_jpeg(blobs, draft=(8, 8), **ALL)
    assert list(pre.last_routes) == ["host", "host"]
    for g, b in zip(got, blobs):
        im = Image.open(io.BytesIO(b))
        im.draft("RGB", (8, 8))
        assert np.array_equal(g.cpu().numpy(), np.asarray(im.convert("RGB")))
    f = L.refused()["Adobe transform 2"][0]
    g, = pre.decode_jpeg([f], **ALL)
    assert pre.last_routes == ("host",) and np.array_equal(g.cpu().numpy(), L.oracle(f))


def test_orientation_tag_6(pre):
    blob = with_orientation(L.CASES["440-17x33"].blob, 6)
    want = np.asarray(Image.fromarray(L.oracle(blob)).transpose(Image.Transpose.ROTATE_270))    # what tag 6 asks for
    assert np.array_equal(want, np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB")))
    got, = pre.decode_jpeg([blob], orientation="exif", **ALL)
    assert pre.last_routes == ("device-layout",) and pre.last_orientations == (6,)
    assert want.shape == (17, 33, 3) and np.array_equal(got.cpu().numpy(), want)


def test_layout_decode_stays_inside_its_workspace(pre, monkeypatch):
    """odic_jpeg3_any_decode on one 4:1:0 17x33 file with the workspace, the compressed-data copy, the RGB output and
    `status` each exactly as large as asked for inside a poisoned allocation: nothing outside them is written."""
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
    name = "410-17x33"
    for knobs in ({}, dict(subseq_bits=32, max_sync_passes=0)):
        got, = fresh.decode_jpeg([L.CASES[name].blob], **ALL, **knobs)
        torch.cuda.synchronize()
        assert fresh.last_routes == ("device-layout",)
        assert np.array_equal(got.cpu().numpy(), L.oracle(L.CASES[name].blob))
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        for g in made:
            g.assert_untouched(what=f"layout decode, {g.dtype} buffer of {g.cols} elements")
        assert len([g for g in made if g.dtype == torch.uint8 and g.cols == 17 * 33 * 3]) == 1
        assert {g.dtype for g in made} == {torch.uint8, torch.int32}
        made.clear()
