"""CPU side of the four-component (CMYK / YCCK) device JPEG route: what `jpeg.parse(..., "convert", cmyk="device")`
admits and refuses, that the defaults stay what they were, the HEADER_ANY_DTYPE record against a ctypes mirror of
odic_jpeg_header_any, the symbols, a numpy model of the colour chain against Pillow, and the batch plan's extra group."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from on_device_image_captioning_amd import jpeg as J

import jpeg_cmyk_cases as K
from jpeg_gray_cases import cmyk_jpeg
from test_jpeg_host import encode, smooth_rgb


@pytest.mark.parametrize("name", K.CASES)
def test_admitted_cases_parse_as_device(name):
    blob, hv, ycck = K.CASES[name]
    with Image.open(io.BytesIO(blob)) as im:
        assert im.mode == "CMYK"
    h = J.parse(blob, "convert", cmyk="device")
    assert h.kind == J.DEVICE, h.reason
    assert h.ncomp == 4 and h.comp_hv == hv and h.ycck is ycck
    assert (h.width, h.height) == Image.open(io.BytesIO(blob)).size
    assert len(h.qtables) == 4 and len(h.dc_tables) == 4 and len(h.ac_tables) == 4
    assert (h.restart_interval > 0) == ("dri" in name)
    assert h.mcus_x == -(-h.width // (8 * hv[0][0])) and h.mcus_y == -(-h.height // (8 * hv[0][1]))


@pytest.mark.parametrize("name", K.refused())
def test_refused_cases_go_to_the_host_with_a_reason(name):
    blob, word = K.refused()[name]
    h = J.parse(blob, "convert", cmyk="device")
    assert h.kind == J.HOST and word in h.reason, h.reason
    assert h.reason != "SOF2"                              # that reason sends a file to parse_progressive


def test_defaults_are_unchanged():
    for blob in (cmyk_jpeg(), K.CASES["ycck-sub2-17x33"][0], K.refused()["progressive (SOF2)"][0]):
        h = J.parse(blob)
        assert h.kind == J.BLACK and h.ncomp == 4
        assert J.parse(blob, "black", cmyk="host") == h
        for h in (J.parse(blob, "convert"), J.parse(blob, "convert", cmyk="host"), J.parse_progressive(blob, "convert")):
            assert h.kind == J.HOST and h.reason == "4 components (CMYK / YCCK)"
    rgb = encode(smooth_rgb(16, 16, seed=1), quality=90)
    a, b = J.parse(rgb, "convert", cmyk="device"), J.parse(rgb)
    assert (a.kind, a.ncomp, a.sampling, a.comp_hv, a.data_offset, a.ycck) == (J.DEVICE, 3, b.sampling, b.comp_hv,
                                                                             b.data_offset, False)


def test_bad_combinations_raise():
    blob = cmyk_jpeg()
    with pytest.raises(ValueError, match="non_rgb"):
        J.parse(blob, cmyk="device")
    with pytest.raises(ValueError, match="non_rgb"):
        J.parse(blob, "black", cmyk="device")
    for bad in ("gpu", "", None, True):
        with pytest.raises(ValueError, match="cmyk"):
            J.parse(blob, "convert", cmyk=bad)


class HeaderAny(ctypes.Structure):
    """odic_jpeg_header_any as include/odic_hip.h declares it."""
    _fields_ = [(n, ctypes.c_int64) for n in ("data_off", "data_end", "out_off", "scan_off", "coef_off", "plane_off")] + \
               [(n, ctypes.c_int32) for n in ("int_off", "unit_off", "width", "height", "color", "mcus_x", "mcus_y", "restart",
                                             "n_intervals", "n_units")] + \
               [("h", ctypes.c_int32 * 4), ("v", ctypes.c_int32 * 4), ("ncomp", ctypes.c_int32), ("pad", ctypes.c_int32),
                ("qt", ctypes.c_uint16 * 64 * 4), ("lut", ctypes.c_uint16 * 512 * 8), ("maxcode", ctypes.c_int32 * 18 * 8),
                ("valoff", ctypes.c_int32 * 18 * 8), ("huffval", ctypes.c_uint8 * 256 * 8)]


def test_header_any_record_matches_the_c_struct():
    """The one per-component baseline record (it replaces the four- and the three-component records and their two tests):
    field names, offsets and size against the ctypes mirror, the numbers of the static_assert in csrc/jpeg_decode.hip,
    and the shared prefix at HEADER_DTYPE's offsets."""
    D = J.HEADER_ANY_DTYPE
    assert D.itemsize == ctypes.sizeof(HeaderAny) == 12032               # the static_assert in csrc/jpeg_decode.hip
    assert list(D.names) == [n for n, _ in HeaderAny._fields_]
    for name, _ in HeaderAny._fields_:
        dt, off = D.fields[name][:2]
        f = getattr(HeaderAny, name)
        assert (off, dt.itemsize) == (f.offset, f.size), name
    assert (D.fields["h"][1], D.fields["ncomp"][1], D.fields["qt"][1], D.fields["huffval"][1]) == (88, 120, 128, 9984)
    # the fields both records have sit at the same offsets up to `sampling` / `color`, and the five behind it too, so the
    # templated kernels read alike
    for name in J.HEADER_DTYPE.names[:10] + J.HEADER_DTYPE.names[11:16]:
        assert D.fields[name][1] == J.HEADER_DTYPE.fields[name][1]
    assert D.names[10] == "color" and D.fields["color"][1] == J.HEADER_DTYPE.fields["sampling"][1]
    assert J.HEADER_DTYPE.itemsize == 9016
    # one rule for the word and the frame in both per-component records
    P = J.PROG_HEADER_ANY_DTYPE
    assert all(D.fields[n][0] == P.fields[n][0] for n in ("color", "ncomp", "h", "v", "qt"))
    assert D.fields["v"][1] - D.fields["h"][1] == 16 == D.fields["ncomp"][1] - D.fields["v"][1]


REMOVED = ("odic_jpeg4_workspace_bytes", "odic_jpeg4_decode", "odic_jpeg4_decode_scaled", "odic_jpeg3_any_workspace_bytes",
           "odic_jpeg3_any_decode", "odic_jpeg3_any_decode_scaled")


def test_abi_version_and_new_symbols():
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    assert lib.odic_abi_version() == 27 == _hip.ABI_VERSION
    for name in ("odic_jpeg_any_workspace_bytes", "odic_jpeg_any_decode", "odic_cmyk_to_rgb8"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.odic_jpeg_any_decode(None, None, 0, None) == -2
    assert lib.odic_jpeg_any_workspace_bytes(None) == 0
    assert lib.odic_cmyk_to_rgb8(None, None, 4, 1, None) == -2
    assert lib.odic_cmyk_to_rgb8(16, 16, -1, 1, None) == -1
    assert lib.odic_cmyk_to_rgb8(16, 16, 0, 1, None) == 0                  # nothing to do, nothing launched
    with open(_hip.LIB_PATH.replace("on_device_image_captioning_amd/libodic_hip.so", "include/odic_hip.h")) as f:
        header = f.read()
    assert "#define ODIC_ABI_VERSION 27" in header and "} odic_jpeg_header_any;" in header
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in REMOVED:                                                  # gone from the library, the table and the header
        assert name not in _hip.EXPORTED_SYMBOLS and not hasattr(raw, name) and name + "(" not in header


def test_cmyk_to_rgb_model_is_pillows_on_every_pair():
    x, k = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    for pos in range(3):
        px = np.zeros((256, 256, 4), np.uint8)
        px[..., pos], px[..., 3] = x, k
        px[..., (pos + 1) % 3] = 255 - x
        want = np.asarray(Image.fromarray(px, "CMYK").convert("RGB"))
        assert np.array_equal(K.cmyk_to_rgb_model(px), want), pos


@pytest.mark.parametrize("name", K.CASES)
def test_color_model_on_pillows_planes_is_pillows_rgb(name):
    """Pillow's CMYK array is libjpeg's output (YCCK already turned into CMYK) with every sample complemented."""
    blob = K.CASES[name][0]
    stored = 255 - np.asarray(Image.open(io.BytesIO(blob)))
    assert np.array_equal(K.color_model(stored, ycck=False), K.oracle(blob))


@pytest.mark.parametrize("size", ["1x1", "7x9", "17x33", "48x64"])
def test_ycck_model_is_libjpegs(size):
    """Without sub-sampling the planes a CMYK file stores are what its YCCK twin stores: the model's YCCK → CMYK on them
    is what libjpeg makes of the twin."""
    stored = 255 - np.asarray(Image.open(io.BytesIO(K.CASES[f"cmyk-sub0-{size}"][0])))
    twin = K.CASES[f"ycck-sub0-{size}"][0]
    assert np.array_equal(K.color_model(stored, ycck=True), K.oracle(twin))
    if size != "1x1":
        assert not np.array_equal(K.oracle(twin), K.oracle(K.CASES[f"cmyk-sub0-{size}"][0]))


BASE = [encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=0)]


def test_batch_plan_lists_the_group_only_when_a_file_is_there():
    hdrs = [J.parse(b) for b in BASE]
    names = ["cmyk-sub2-17x33", "photoshop-ycck-2x2-7x9"]
    cblobs = [K.CASES[n][0] for n in names]
    chdrs = [J.parse(b, "convert", cmyk="device") for b in cblobs]
    plain = J.plan_device_batch([("base", hdrs, BASE)], 2048, [1])
    same = J.plan_device_batch([("base", hdrs, BASE), ("prog", [], []), ("own", [], []), ("pany", [], [])], 2048, [1])
    assert plain.group("own") is None and [g.kind for g in plain.groups] == ["base"] == [g.kind for g in same.groups]
    assert [a.dtype for _, a in plain.sections] == [J.HEADER_DTYPE]
    host_a, host_b = np.zeros(plain.total, np.uint8), np.zeros(same.total, np.uint8)
    plain.fill(host_a)
    same.fill(host_b)
    assert plain.total == same.total and np.array_equal(host_a, host_b) and plain.out_offs == same.out_offs

    for base_h, base_b in ((hdrs, BASE), ([], [])):
        p = J.plan_device_batch([("base", base_h, base_b), ("own", chdrs, cblobs)], 2048, [1] * len(base_h))
        g = p.group("own")
        assert (g.n, g.first) == (2, len(base_h))
        assert [a.dtype for _, a in p.sections] == [J.HEADER_DTYPE] * len(base_h) + [J.HEADER_ANY_DTYPE]
        spans = [(o, o + a.nbytes) for o, a in p.sections] + [(p.data_off, p.total)]
        assert all(lo % 256 == 0 for lo, _ in spans) and spans == sorted(spans)
        assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]))
        assert (p.sections[-1][0],) == g.offs
        host = np.full(p.total + 16, 0xA5, np.uint8)
        p.fill(host)
        assert (host[p.total:] == 0xA5).all()
        rec = host[g.offs[0]:g.offs[0] + 2 * J.HEADER_ANY_DTYPE.itemsize].view(J.HEADER_ANY_DTYPE)
        nb = len(base_h)
        for r, h, (o, _), blob in zip(rec, chdrs, p.blobs[nb:], cblobs):
            lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
            assert (lo, hi) == (o + h.data_offset, o + len(blob)) and host[lo:hi].tobytes() == blob[h.data_offset:]
            assert list(zip(r["h"], r["v"])) == h.comp_hv and bool(r["color"]) == h.ycck and r["ncomp"] == 4
            assert int(r["out_off"]) % 4 == 0
        # the output: the group starts on a multiple of 256 behind the others' bytes, images do not overlap
        assert g.out_off % 256 == 0 and g.out_off >= p.out_bytes + p.pout_bytes
        assert p.out_offs[nb:] == [g.out_off + int(o) for o in rec["out_off"]]
        ends = [o + h.width * h.height * 3 for o, h in zip(p.out_offs[nb:], chdrs)]
        assert all(e <= o for e, o in zip(ends, p.out_offs[nb + 1:])) and ends[-1] == g.out_off + g.out_bytes
        # workspace totals: 64 plane bytes and one coefficient block per block of every component
        blocks = [h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv) for h in chdrs]
        assert g.tot["total_blocks"] == sum(blocks) and g.tot["total_plane_bytes"] == 64 * sum(blocks)
        assert g.tot["max_blocks"] == max(blocks)
