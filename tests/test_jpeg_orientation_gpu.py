"""`orientation="exif"` end to end on the GPU: DevicePreprocessor.decode_jpeg / from_jpeg_bytes / from_files against
`ImageOps.exif_transpose` and against the host path, bit for bit; the routes stay on the device; and the default,
unchanged and without a call of odic_orient_rgb8."""
import io
import warnings

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import jpeg_exif_cases as X

pytestmark = pytest.mark.gpu

SIZES = [(37, 23), (100, 75)]                                           # (width, height), no MCU multiples
ROUTE = {"444": "device", "420_dri": "device", "writer": "device", "gray": "device", "progressive": "device-progressive",
         "gray_progressive": "device-progressive"}
EXIF = dict(progressive="device", non_rgb="convert", orientation="exif")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(32, "cuda:0", max_pixels=1024 * 512)


def upright(blob):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB"))


def stored(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def batch(kind, size):
    """Orientations 1..8, the XMP-only and the two-APP1 files and one without APP1, of one kind and size."""
    base = X.base_file(kind, size, seed=len(kind))
    blobs = [X.with_orientation(base, o) for o in range(1, 9)]
    blobs += [X.TAG_CASES[n][0](base) for n in ("xmp_attr_8", "two_exif_6_then_3", "ascii_6")] + [base]
    return blobs, [1, 2, 3, 4, 5, 6, 7, 8, 8, 6, 1, 1]


def no_host(pre, monkeypatch):
    def boom(*a, **kw):
        raise AssertionError("host decode")
    monkeypatch.setattr(pre, "_host_rgb", boom)


@pytest.mark.parametrize("size", SIZES, ids=["37x23", "100x75"])
@pytest.mark.parametrize("kind", list(ROUTE))
def test_decode_jpeg_equals_exif_transpose(pre, monkeypatch, kind, size):
    blobs, turns = batch(kind, size)
    no_host(pre, monkeypatch)                                           # orientation never turns a device route into a host one
    got = pre.decode_jpeg(blobs, **EXIF)
    assert pre.last_routes == (ROUTE[kind],) * len(blobs)
    assert pre.last_orientations == tuple(turns)
    for k, (g, b) in enumerate(zip(got, blobs)):
        w = upright(b)
        assert tuple(g.shape) == w.shape, (k, tuple(g.shape), w.shape)
        assert g.is_contiguous() and np.array_equal(g.cpu().numpy(), w), k


@pytest.mark.parametrize("kind", list(ROUTE))
def test_ignore_decodes_as_before_without_the_orient_kernel(pre, monkeypatch, kind):
    """The default: the stored grid, and the library is never asked to orient.  Holds with and without the feature."""
    blobs, _ = batch(kind, SIZES[0])
    no_host(pre, monkeypatch)

    class Spy:
        def __init__(self, lib):
            self._lib, self.calls = lib, []

        def __getattr__(self, name):
            self.calls.append(name)
            return getattr(self._lib, name)

    spy = Spy(pre.lib)
    monkeypatch.setattr(pre, "lib", spy)
    for kw in (dict(), dict(orientation="ignore")):
        try:
            got = pre.decode_jpeg(blobs, progressive="device", non_rgb="convert", **kw)
        except TypeError:                                               # a version without the argument: its default
            assert kw
            continue
        for g, b in zip(got, blobs):
            assert np.array_equal(g.cpu().numpy(), stored(b))
        assert pre.last_routes == (ROUTE[kind],) * len(blobs)
        assert tuple(getattr(pre, "last_orientations", (1,) * len(blobs))) == (1,) * len(blobs)
    assert spy.calls and "odic_orient_rgb8" not in spy.calls


def write(tmp_path, blobs):
    paths = []
    for k, b in enumerate(blobs):
        (tmp_path / f"f{k}.jpg").write_bytes(b)
        paths.append(str(tmp_path / f"f{k}.jpg"))
    return paths


def test_from_jpeg_bytes_equals_the_host_path(pre, tmp_path):
    blobs = []
    for kind in ("444", "420_dri", "writer"):
        blobs += batch(kind, (100, 75))[0][3:9]
    paths = write(tmp_path, blobs)
    host = pre.from_files(paths, orientation="exif")
    assert torch.equal(pre.from_jpeg_bytes(blobs, orientation="exif"), host)
    assert torch.equal(pre.from_files(paths, decode="device", orientation="exif"), host)
    assert pre.last_routes == ("device",) * len(blobs)
    assert not torch.equal(host, pre.from_files(paths))                # and the tag does change the tensor


def test_draft_then_orientation(pre, tmp_path):
    """1000 x 400 at S = 32: Pillow's draft picks 1/8, then exif_transpose turns the 125 x 50 image."""
    base = X.base_file("420_dri", (1000, 400), seed=5)
    blobs = [X.with_orientation(base, o) for o in (1, 3, 6, 7)] + [X.with_orientation(X.base_file("progressive", (1000, 400)), 8)]
    got = pre.decode_jpeg(blobs, draft=(32, 32), progressive="device", orientation="exif")
    assert [tuple(g.shape) for g in got] == [(50, 125, 3), (50, 125, 3), (125, 50, 3), (125, 50, 3), (125, 50, 3)]
    for g, b in zip(got, blobs):
        im = Image.open(io.BytesIO(b))
        im.draft("RGB", (32, 32))
        assert np.array_equal(g.cpu().numpy(), np.asarray(ImageOps.exif_transpose(im)))
    paths = write(tmp_path, blobs)
    host = pre.from_files(paths, draft=True, orientation="exif")
    assert torch.equal(pre.from_jpeg_bytes(blobs, progressive="device", draft=True, orientation="exif"), host)
    assert pre.last_routes == ("device",) * 4 + ("device-progressive",)


def test_regions_on_a_mixed_batch_are_in_oriented_coordinates(pre, tmp_path):
    """Oriented images live in the orient launch's buffer, unoriented ones in the decoder's: one region call over both."""
    base = X.base_file("444", (100, 75), seed=6)
    blobs = [base, X.with_orientation(base, 6), X.with_orientation(base, 1), X.with_orientation(base, 2),
             X.with_orientation(X.base_file("420_dri", (37, 23)), 5)]
    regions = [(0, (10, 5, 90.5, 70)), (1, (0, 0, 75, 100)), (1, (5.5, 60, 70, 99)), (2, (0, 0, 100, 75)),
               (3, (50, 10, 100, 75)), (4, (0, 0, 23, 37)), (4, (3, 20, 20.25, 36)), (0, (0, 0, 100, 75))]
    paths = write(tmp_path, blobs)
    host = pre.from_files(paths, regions=regions, orientation="exif")
    assert torch.equal(pre.from_jpeg_bytes(blobs, regions=regions, orientation="exif"), host)
    assert pre.last_orientations == (1, 6, 1, 2, 5)
    with pytest.raises(ValueError):                                     # a box of the stored grid does not fit the upright image
        pre.from_jpeg_bytes(blobs, regions=[(1, (0, 0, 100, 75))], orientation="exif")


def test_black_canvas_has_the_transposed_shape(pre, tmp_path):
    base = X.base_file("gray", (37, 23))
    blobs = [X.with_orientation(base, 6), X.with_orientation(base, 3), X.with_orientation(X.base_file("444", (37, 23)), 6)]
    got = pre.decode_jpeg(blobs, orientation="exif")                    # non_rgb="black", the default
    assert pre.last_routes == ("black", "black", "device") and pre.last_orientations == (6, 3, 6)
    assert [tuple(g.shape) for g in got] == [(37, 23, 3), (23, 37, 3), (37, 23, 3)]
    assert not got[0].any() and not got[1].any() and got[2].any()
    paths = write(tmp_path, blobs)
    regions = [(0, (0, 0, 23, 37)), (2, (0, 0, 23, 37))]
    for kw in (dict(), dict(regions=regions)):
        assert torch.equal(pre.from_jpeg_bytes(blobs, orientation="exif", **kw),
                           pre.from_files(paths, orientation="exif", **kw))


def test_files_pil_decodes_are_turned_by_pil(pre, tmp_path):
    """A PNG with EXIF and a CMYK JPEG go to the host route and come back upright; a status fallback too."""
    exif = Image.open(io.BytesIO(X.with_orientation(X.base_file("444"), 5))).getexif().tobytes()
    png = io.BytesIO()
    Image.fromarray(X.smooth_rgb(20, 30)).save(png, format="PNG", exif=exif)
    cmyk = io.BytesIO()
    Image.fromarray(X.smooth_rgb(20, 30)).convert("CMYK").save(cmyk, format="JPEG")
    blobs = [png.getvalue(), X.with_orientation(cmyk.getvalue(), 8), X.with_orientation(X.base_file("444"), 4)]
    got = pre.decode_jpeg(blobs, non_rgb="convert", orientation="exif")
    assert pre.last_routes == ("host", "host", "device") and pre.last_orientations == (5, 8, 4)
    for g, b in zip(got, blobs):
        assert np.array_equal(g.cpu().numpy(), upright(b))
    paths = write(tmp_path, blobs)
    for kw in (dict(non_rgb="convert"), dict()):
        assert torch.equal(pre.from_jpeg_bytes(blobs, orientation="exif", **kw),
                           pre.from_files(paths, orientation="exif", **kw))
