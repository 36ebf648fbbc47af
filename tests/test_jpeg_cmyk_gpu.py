"""Four-component (CMYK / YCCK) JPEGs on the device: `decode_jpeg(..., non_rgb="convert", cmyk="device")` against
`np.asarray(Image.open(f).convert("RGB"))` bit for bit, the conversion stage on its own over every (x, K) pair, a mixed
batch, the status fallback, EXIF orientation, and the containment of odic_jpeg_any_decode."""
import io

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import jpeg_cmyk_cases as K
from guards import POISON, guarded
from jpeg_exif_cases import with_orientation
from jpeg_gray_cases import gray_file, png, truncated
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

KNOBS = {"default": dict(), "subseq32": dict(subseq_bits=32), "serial": dict(max_sync_passes=0),
         "subseq32-serial": dict(subseq_bits=32, max_sync_passes=0)}
DEVICE = dict(non_rgb="convert", cmyk="device")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


@pytest.fixture(scope="module")
def oracles():
    return {name: torch.from_numpy(K.oracle(blob).copy()) for name, (blob, _, _) in K.CASES.items()}


@pytest.mark.parametrize("invert", [0, 1])
def test_cmyk_to_rgb8_on_every_pair(pre, invert):
    """All 65 536 (x, K) pairs in each of the three channel positions (the other two channels hold 255 - x and x ^ K)."""
    x, k = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    px = np.zeros((3, 256, 256, 4), np.uint8)
    for pos in range(3):
        px[pos, ..., pos], px[pos, ..., (pos + 1) % 3], px[pos, ..., (pos + 2) % 3], px[pos, ..., 3] = x, 255 - x, x ^ k, k
    flat = px.reshape(-1, 4)
    want = np.asarray(Image.frombytes("CMYK", (flat.shape[0], 1), (255 - flat if invert else flat).tobytes()).convert("RGB"))
    for n, shift in ((flat.shape[0], 0), (1, 0), (7, 4)):    # whole, one pixel, an odd count from a source that is not 16-aligned
        src = torch.from_numpy(flat[:n + shift // 4].copy()).to("cuda:0").view(-1)[shift:shift + 4 * n]
        dst = guarded(1, 3 * n, 3 * n, torch.uint8, "cuda:0")
        pre._hip.check(pre.lib.odic_cmyk_to_rgb8(src.data_ptr(), dst.t.data_ptr(), n, invert,
                                                 torch.cuda.current_stream().cuda_stream), "odic_cmyk_to_rgb8")
        torch.cuda.synchronize()
        dst.assert_untouched(what="odic_cmyk_to_rgb8")
        first = shift // 4
        assert np.array_equal(dst.t.view(-1)[:3 * n].cpu().numpy().reshape(n, 3), want[0, first:first + n]), (n, shift)


@pytest.mark.parametrize("knobs", KNOBS)
def test_every_case_file(pre, oracles, knobs):
    names = list(K.CASES)
    got = pre.decode_jpeg([K.CASES[n][0] for n in names], **DEVICE, **KNOBS[knobs])
    routes = dict(zip(names, pre.last_routes))
    assert routes == {n: "device-cmyk" for n in names}          # none on the host, none "host-after-status"
    wrong = [n for n, g in zip(names, got) if g.shape != oracles[n].shape or not torch.equal(g.cpu(), oracles[n])]
    assert not wrong, wrong
    for n in names[::9]:                                         # ... and alone
        g, = pre.decode_jpeg([K.CASES[n][0]], **DEVICE, **KNOBS[knobs])
        assert pre.last_routes == ("device-cmyk",) and torch.equal(g.cpu(), oracles[n]), n


def mixed():
    cmyk = K.CASES["cmyk-sub2-48x64"][0]
    prog = K.refused()["progressive (SOF2)"][0]
    blobs = [encode(smooth_rgb(48, 64, seed=1), quality=90, subsampling=2), gray_file("dri3", (37, 53)), cmyk,
             K.CASES["photoshop-ycck-2x2-17x33"][0], png("RGBA", 19, 23), prog]
    return blobs, ["device", "device", "device-cmyk", "device-cmyk", "host", "host"]


def test_mixed_batch(pre):
    blobs, routes = mixed()
    want = [torch.from_numpy(K.oracle(b).copy()) for b in blobs]
    got = pre.decode_jpeg(blobs, **DEVICE)
    assert list(pre.last_routes) == routes
    host = pre.decode_jpeg(blobs, non_rgb="convert", cmyk="host")
    assert list(pre.last_routes) == ["device", "device", "host", "host", "host", "host"]
    for k, (g, h, w) in enumerate(zip(got, host, want)):
        assert torch.equal(g.cpu(), w) and torch.equal(g, h), k
    # under a draft request four-component files stay on the host route, with the host's result
    got = pre.decode_jpeg(blobs[2:4], draft=(8, 8), **DEVICE)
    assert list(pre.last_routes) == ["host", "host"]
    for g, b in zip(got, blobs[2:4]):
        im = Image.open(io.BytesIO(b))
        im.draft("RGB", (8, 8))
        assert np.array_equal(g.cpu().numpy(), np.asarray(im.convert("RGB")))


def test_from_jpeg_bytes_and_regions_equal_the_host_route(pre):
    blobs, _ = mixed()
    a = pre.from_jpeg_bytes(blobs, **DEVICE)
    assert "device-cmyk" in pre.last_routes
    assert torch.equal(a, pre.from_jpeg_bytes(blobs, non_rgb="convert"))
    regions = [(2, (3.5, 2.0, 40.0, 61.25)), (3, (0.0, 1.0, 17.0, 30.5))]
    assert torch.equal(pre.from_jpeg_bytes(blobs, regions=regions, **DEVICE),
                       pre.from_jpeg_bytes(blobs, regions=regions, non_rgb="convert"))
    with pytest.raises(ValueError, match="non_rgb"):
        pre.decode_jpeg(blobs, cmyk="device")
    with pytest.raises(ValueError, match="cmyk"):
        pre.decode_jpeg(blobs, non_rgb="convert", cmyk="gpu")


def test_truncated_ycck_falls_back_to_the_host(pre):
    whole = K.CASES["ycck-sub2-48x64"][0]
    cut = truncated(whole)
    try:
        want = np.asarray(Image.open(io.BytesIO(cut)).convert("RGB"))
    except Exception as e:                                       # the host path's exception is the device path's
        with pytest.raises(type(e)):
            pre.decode_jpeg([whole, cut], **DEVICE)
        assert pre.last_routes == ("device-cmyk", "host-after-status")
        return
    got = pre.decode_jpeg([whole, cut], **DEVICE)
    assert pre.last_routes == ("device-cmyk", "host-after-status")
    assert np.array_equal(got[0].cpu().numpy(), K.oracle(whole)) and np.array_equal(got[1].cpu().numpy(), want)


def test_orientation_tag_6(pre):
    blob = with_orientation(K.CASES["cmyk-sub1-17x33"][0], 6)
    want = np.asarray(Image.fromarray(K.oracle(blob)).transpose(Image.Transpose.ROTATE_270))    # what tag 6 asks for
    assert np.array_equal(want, np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB")))
    got, = pre.decode_jpeg([blob], orientation="exif", **DEVICE)
    assert pre.last_routes == ("device-cmyk",) and pre.last_orientations == (6,)
    assert want.shape == (17, 33, 3) and np.array_equal(got.cpu().numpy(), want)


def test_jpeg4_decode_stays_inside_its_workspace(pre, monkeypatch):
    """odic_jpeg_any_decode on a two-image batch with the workspace, the compressed-data copy, the RGB output and `status` each
    exactly as large as asked for inside a poisoned allocation: nothing outside them is written, nor are the bytes of the
    output that lie between the images (the second image's offset is rounded up to a multiple of 4)."""
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
    names = ["photoshop-ycck-2x2-7x9", "cmyk-sub2-dri3"]        # 7·9·3 = 189 bytes: the second image starts at 192
    for knobs in ({}, dict(subseq_bits=32, max_sync_passes=0)):
        got = fresh.decode_jpeg([K.CASES[n][0] for n in names], **DEVICE, **knobs)
        torch.cuda.synchronize()
        assert fresh.last_routes == ("device-cmyk", "device-cmyk")
        for n, g in zip(names, got):
            assert np.array_equal(g.cpu().numpy(), K.oracle(K.CASES[n][0])), n
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        for g in made:
            g.assert_untouched(what=f"jpeg4 decode, {g.dtype} buffer of {g.cols} elements")
        rgb = [g for g in made if g.dtype == torch.uint8 and g.cols == 192 + 48 * 64 * 3]
        assert len(rgb) == 1
        assert (rgb[0].t.view(-1)[189:192].cpu().numpy() == POISON).all()
        assert {g.dtype for g in made} == {torch.uint8, torch.int32}
        made.clear()
