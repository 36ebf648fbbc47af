"""EXIF orientation without a GPU: `jpeg.exif_orientation` against Pillow on hand-built APP1 segments, the parsers on
files that carry them, `jpeg.orient_box`, the host route of `DevicePreprocessor` and the C entry's argument checks."""
import ctypes
import dataclasses
import io
import os
import re
import warnings

import numpy as np
import pytest
from PIL import Image, ImageOps

import jpeg_exif_cases as X
from on_device_image_captioning_amd import image_utils as IU
from on_device_image_captioning_amd import jpeg as J
from test_regions_host import c_struct_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "odic_hip.h")


def pil(blob):
    return Image.open(io.BytesIO(blob))


def transposed(im, orientation):
    return im if orientation == 1 else im.transpose(J.transpose_method(orientation))


# ------------------------------------------------------------------------------------------------------ the tag reader
@pytest.mark.parametrize("name", list(X.TAG_CASES))
def test_exif_orientation_equals_pillows_effective_orientation(name):
    """Every row of the table: first that the installed Pillow does with the bytes what the table says (the tag it reports,
    the transposition exif_transpose applies), then that the reader returns that orientation."""
    make, tag, effective = X.TAG_CASES[name]
    blob = make(X.base_file("444", (37, 23)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert X.pillow_tag(blob) == tag and type(X.pillow_tag(blob)) is type(tag)
        want = np.asarray(ImageOps.exif_transpose(pil(blob)))
    assert np.array_equal(want, np.asarray(transposed(pil(blob), effective)))
    if effective != 1:                                                  # and no other orientation gives that array
        assert not np.array_equal(want, np.asarray(pil(blob)))
    assert J.exif_orientation(blob) == effective
    assert J.exif_orientation(memoryview(blob)) == effective


@pytest.mark.parametrize("kind", X.KINDS)
def test_exif_orientation_on_every_kind_of_file(kind):
    """One-component, SOF2 and hand-written files, with and without APP1."""
    base = X.base_file(kind, (100, 75), seed=2)
    assert J.exif_orientation(base) == 1
    for name in ("plain_6", "long_MM_6", "xmp_attr_8", "two_exif_6_then_3", "ascii_6"):
        make, _, effective = X.TAG_CASES[name]
        blob = make(base)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = ImageOps.exif_transpose(pil(blob))
        assert want.size == J.oriented_size(pil(blob).size, effective), (kind, name)
        assert J.exif_orientation(blob) == effective, (kind, name)


def test_exif_orientation_never_raises():
    assert J.exif_orientation(b"") == 1 and J.exif_orientation(b"not an image at all") == 1
    blob = X.with_orientation(X.base_file("444"), 6)
    assert J.exif_orientation(blob[:len(blob) // 3]) in (1, 6)         # cut inside the tables: Pillow's word, no raise
    png = io.BytesIO()
    Image.fromarray(X.smooth_rgb(9, 14)).save(png, format="PNG", exif=pil(blob).getexif().tobytes())
    assert J.exif_orientation(png.getvalue()) == J.pil_orientation(pil(png.getvalue())) == 6      # any format: Pillow


# --------------------------------------------------------------------------------------------------------- the parsers
def _fields(h, skip=("data_offset", "scans", "app1")):
    return {f.name: getattr(h, f.name) for f in dataclasses.fields(h) if f.name not in skip}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if k == "qtables":
            assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
        else:
            assert x == y, k


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("name", ["plain_6", "two_exif_6_then_3", "exif_no_tag_xmp_element_5", "app1_before_app0"])
def test_parsers_read_the_same_headers_with_exif(kind, name):
    base = X.base_file(kind, (37, 23), seed=1)
    blob = X.TAG_CASES[name][0](base)
    shift = len(blob) - len(base)
    assert shift > 0
    for opt in ("black", "convert"):
        a, b = J.parse(base, opt), J.parse(blob, opt)
        _same(_fields(a), _fields(b))
        assert b.data_offset == (a.data_offset + shift if a.kind == J.DEVICE else 0)
        assert J.header_orientation(b, blob) == J.exif_orientation(blob) == X.TAG_CASES[name][2]
        if a.kind == J.HOST and a.reason == "SOF2":
            pa, pb = J.parse_progressive(base, opt), J.parse_progressive(blob, opt)
            _same(_fields(pa), _fields(pb))
            assert J.header_orientation(pb, blob) == X.TAG_CASES[name][2]
            assert len(pa.scans) == len(pb.scans)
            for sa, sb in zip(pa.scans, pb.scans):
                da, db = dataclasses.asdict(sa), dataclasses.asdict(sb)
                assert db.pop("data_offset") == da.pop("data_offset") + shift
                assert db.pop("data_end") == da.pop("data_end") + shift
                assert da == db


# ---------------------------------------------------------------------------------------------------------- orient_box
@pytest.mark.parametrize("o", range(1, 9))
def test_orient_box_round_trips(o):
    size = (31, 17)
    for box in ((0, 0, 31, 17), (3, 2, 10, 9), (0.25, 1.5, 30.75, 16.0), (30, 16, 31, 17)):
        there = J.orient_box(box, size, o)
        ow, oh = J.oriented_size(size, o)
        assert 0 <= there[0] < there[2] <= ow and 0 <= there[1] < there[3] <= oh
        assert J.orient_box(there, size, o, inverse=True) == tuple(box)
    with pytest.raises(ValueError):
        J.orient_box((0, 0, 1, 1), size, 9)


@pytest.mark.parametrize("o", range(1, 9))
def test_orient_box_agrees_with_pil(o):
    """Paint a box in an image, transpose with PIL, find it again."""
    w, h = 31, 17
    box = (4, 2, 13, 7)
    a = np.zeros((h, w, 3), np.uint8)
    a[box[1]:box[3], box[0]:box[2]] = 255
    t = np.asarray(transposed(Image.fromarray(a), o))[:, :, 0]
    ys, xs = np.nonzero(t)
    found = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
    assert J.orient_box(box, (w, h), o) == found
    assert J.orient_box(found, (w, h), o, inverse=True) == box


# ------------------------------------------------------------------------------------------------------ the host route
@pytest.mark.parametrize("kind", ["444", "gray", "progressive"])
def test_host_route_is_exif_transpose_after_draft_and_non_rgb_rule(kind):
    pre = object.__new__(IU.DevicePreprocessor)
    base = X.base_file(kind, (100, 75), seed=4)
    for o in range(1, 9):
        blob = X.with_orientation(base, o)
        for draft in (None, (20, 20)):
            im = pil(blob)
            if draft:
                im.draft("RGB", draft)
            up = ImageOps.exif_transpose(im)
            conv = np.asarray(up.convert("RGB"))
            black = conv if up.mode == "RGB" else np.zeros_like(conv)
            assert np.array_equal(pre._host_rgb(blob, draft, "convert", orientation="exif"), conv), (o, draft)
            assert np.array_equal(pre._host_rgb(blob, draft, orientation="exif"), black), (o, draft)
            stored = pil(blob)
            if draft:
                stored.draft("RGB", draft)
            assert np.array_equal(pre._host_rgb(blob, draft, "convert"), np.asarray(stored.convert("RGB")))     # ignore


def test_unknown_orientation_is_a_value_error(tmp_path):
    pre = object.__new__(IU.DevicePreprocessor)
    blob = X.base_file("444")
    (tmp_path / "a.jpg").write_bytes(blob)
    for decode in ("host", "device"):
        with pytest.raises(ValueError, match="orientation"):
            pre.from_files([str(tmp_path / "a.jpg")], decode=decode, orientation="upright")
    with pytest.raises(ValueError, match="orientation"):
        pre.decode_jpeg([blob], orientation="EXIF")
    with pytest.raises(ValueError, match="orientation"):
        pre.from_jpeg_bytes([blob], orientation=6)
    with pytest.raises(ValueError, match="orientation"):
        J.check_orientation(None)


# --------------------------------------------------------------------------------------------------------- the C entry
@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_abi_stays_26_and_header_and_binding_agree(lib):
    from on_device_image_captioning_amd import _hip
    text = open(HEADER).read()
    assert _hip.ABI_VERSION == 27 == lib.odic_abi_version() and re.search(r"#define ODIC_ABI_VERSION 27\b", text)
    assert "odic_orient_rgb8" in _hip.EXPORTED_SYMBOLS and hasattr(ctypes.CDLL(_hip.LIB_PATH), "odic_orient_rgb8")
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    proto = re.search(r"int odic_orient_rgb8\((.*?)\);", bare, flags=re.S).group(1)
    assert len(proto.split(",")) == len(_hip._SIGNATURES["odic_orient_rgb8"][1]) == 5


def test_job_record_matches_the_c_struct():
    fields = c_struct_fields("odic_orient_job")
    assert [n for _, n in fields] == list(IU.ORIENT_JOB_DTYPE.names)
    ctypes_of = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}

    class Job(ctypes.Structure):                                        # the C compiler's layout rules
        _fields_ = [(n, ctypes_of[t]) for t, n in fields]

    assert IU.ORIENT_JOB_DTYPE.itemsize == ctypes.sizeof(Job) == 40    # sizeof(odic_orient_job), static_assert in the HIP
    for t, n in fields:
        assert IU.ORIENT_JOB_DTYPE.fields[n][1] == getattr(Job, n).offset, n
        assert IU.ORIENT_JOB_DTYPE.fields[n][0].itemsize == ctypes.sizeof(ctypes_of[t]), n


def test_argument_refusals_need_no_gpu(lib):
    good = dict(src_off=0, dst_off=0, src_stride_bytes=21, H=5, W=7, orientation=6)

    def call(n=2, src=16, dst=1 << 20, null_jobs=False, **kw):
        rec = np.zeros(2, IU.ORIENT_JOB_DTYPE)
        for k, v in good.items():
            rec[k] = v
        for k, v in kw.items():
            rec[k][1] = v                                               # the second job: the first one is fine
        return lib.odic_orient_rgb8(None if null_jobs else rec.ctypes.data, n, src, dst, None)

    assert call(n=-1) == -1                                             # ODIC_EINVAL, all of them, before any launch
    assert call(null_jobs=True) == -1 and call(src=None) == -1 and call(dst=None) == -1
    for kw in (dict(orientation=1), dict(orientation=0), dict(orientation=9), dict(orientation=-6), dict(H=0), dict(H=-5),
               dict(W=0), dict(W=-7), dict(src_stride_bytes=20), dict(src_stride_bytes=-21)):
        assert call(**kw) == -1, kw
    assert call(n=0) == 0 and call(n=0, null_jobs=True, src=None, dst=None) == 0          # nothing to do, nothing launched
