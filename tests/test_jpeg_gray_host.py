"""CPU side of `non_rgb="convert"`: the option's validation, what `jpeg.parse` / `jpeg.parse_progressive` make of
one- and four-component frames with and without it, the batch plan of a call that mixes gray and colour files, and the
host route (`DevicePreprocessor._pil_rgb`) against Pillow's `convert("RGB")`."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_gray_cases as G
from on_device_image_captioning_amd import jpeg as J
from on_device_image_captioning_amd.image_utils import DevicePreprocessor
from test_jpeg_host import encode, smooth_rgb

SIZE = (37, 53)


def same_header(a, b):
    """Everything the packers read, but for where the scan data starts."""
    keys = ("kind", "width", "height", "ncomp", "sampling", "comp_hv", "restart_interval", "mcus_x", "mcus_y")
    assert [getattr(a, k) for k in keys] == [getattr(b, k) for k in keys]
    assert all(np.array_equal(x, y) for x, y in zip(a.qtables, b.qtables)) and len(a.qtables) == len(b.qtables) == 1
    return True


# ---------------------------------------------------------------------------------------------------------------
# the option
# ---------------------------------------------------------------------------------------------------------------
def test_option_is_validated_by_the_parsers():
    blob = G.gray_file("baseline", (8, 8))
    for fn in (J.parse, J.parse_progressive):
        with pytest.raises(ValueError, match="non_rgb"):
            fn(blob, non_rgb="nonsense")
        with pytest.raises(ValueError, match="non_rgb"):
            fn(blob, "gray")
        assert fn(blob, non_rgb="black").kind == fn(blob).kind


@pytest.mark.parametrize("entry", ["from_files", "from_jpeg_bytes", "decode_jpeg"])
def test_option_is_validated_before_any_device_work(entry):
    """The entry points reject the value before they touch the device: an object that never was initialised will do."""
    pre = object.__new__(DevicePreprocessor)
    with pytest.raises(ValueError, match="non_rgb"):
        getattr(pre, entry)([], non_rgb="nonsense")
    with pytest.raises(ValueError, match="non_rgb"):
        getattr(pre, entry)([], non_rgb=None)


def test_default_parsing_is_unchanged():
    for kind in G.KINDS:
        blob = G.gray_file(kind, SIZE)
        for hd in (J.parse(blob), J.parse_progressive(blob), J.parse(blob, "black")):
            assert hd.kind == J.BLACK and (hd.width, hd.height, hd.ncomp) == SIZE + (1,)
    cmyk = G.cmyk_jpeg()
    assert J.parse(cmyk).kind == J.BLACK and J.parse(cmyk).ncomp == 4
    rgb = encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=2)
    a, b = J.parse(rgb), J.parse(rgb, "convert")                  # three components: the option changes nothing
    assert a.kind == b.kind == J.DEVICE and a.sampling == b.sampling == 2 and a.data_offset == b.data_offset


# ---------------------------------------------------------------------------------------------------------------
# parsing under the option
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", G.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["baseline", "optimize", "dri1", "dri3"])
def test_gray_baseline_is_a_device_kind(kind, size):
    blob = G.gray_file(kind, size)
    hd = J.parse(blob, "convert")
    w, h = size
    assert hd.kind == J.DEVICE and not isinstance(hd, J.ProgHeader), hd.reason
    assert (hd.width, hd.height, hd.ncomp, hd.sampling) == (w, h, 1, 3) and J.GRAY == 3
    assert (hd.mcus_x, hd.mcus_y) == (-(-w // 8), -(-h // 8))                    # the non-interleaved geometry
    assert len(hd.qtables) == len(hd.dc_tables) == len(hd.ac_tables) == 1
    blocks = hd.mcus_x * hd.mcus_y
    r = {"dri1": 1, "dri3": 3}.get(kind, 0)
    assert hd.restart_interval == r                                              # a restart interval counts blocks
    assert J.n_intervals(hd) == (-(-blocks // r) if r else 1)
    assert blob[hd.data_offset - 6:hd.data_offset - 5] == b"\x01" and blob[-2:] == b"\xff\xd9"
    assert J.parse_progressive(blob, "convert").kind == J.HOST                   # SOF0: `parse` takes those


def test_restart_3_on_37x53_wraps_the_marker_numbers():
    hd = J.parse(G.gray_file("dri3", SIZE), "convert")
    assert hd.mcus_x * hd.mcus_y == 35 and J.n_intervals(hd) == 12


@pytest.mark.parametrize("kind", ["progressive", "progressive-dri3"])
def test_gray_progressive_is_a_device_kind(kind):
    blob = G.gray_file(kind, SIZE)
    first = J.parse(blob, "convert")
    assert first.kind == J.HOST and first.reason == "SOF2"                       # what decode_jpeg keys on
    hd = J.parse_progressive(blob, "convert")
    assert hd.kind == J.DEVICE and isinstance(hd, J.ProgHeader), hd.reason
    assert (hd.width, hd.height, hd.ncomp, hd.sampling, hd.mcus_x, hd.mcus_y) == SIZE + (1, 3, 5, 7)
    assert len(hd.scans) >= 2
    for s in hd.scans:                                                           # every scan is non-interleaved
        assert s.comps == [0] and (s.blocks_w, s.n_units) == (5, 35)
        assert s.restart_interval == (3 if kind.endswith("dri3") else 0)
        assert s.n_intervals == (12 if kind.endswith("dri3") else 1)
        assert blob[s.data_end] == 0xFF and blob[s.data_end + 1] in (0xC4, 0xDA, 0xD9)
    dc = [s for s in hd.scans if s.ss == 0]
    assert dc[0].level == 1 and dc[0].dc_tables[0] is not None
    assert all(s.level > 1 for s in hd.scans[1:])                                # all follow the first DC scan
    assert hd.n_levels == max(s.level for s in hd.scans)


@pytest.mark.parametrize("kind", ["baseline", "dri3", "progressive"])
def test_patched_sampling_factors_and_ids_parse_to_the_same_header(kind):
    blob = G.gray_file(kind, SIZE)
    parse = J.parse_progressive if kind == "progressive" else J.parse
    ref = parse(blob, "convert")
    assert ref.kind == J.DEVICE
    for hv in G.HV_PATCHES:
        patched = G.patch_hv(blob, hv)
        assert patched != blob and len(patched) == len(blob)
        hd = parse(patched, "convert")
        assert same_header(hd, ref) and hd.comp_ids == ref.comp_ids
    patched = G.patch_id(blob)
    hd = parse(patched, "convert")
    assert same_header(hd, ref) and hd.comp_ids == [G.PATCHED_ID] != ref.comp_ids
    # the scan must name that id
    only_sof = bytearray(blob)
    sof = [s for s in G.segments(blob) if s[0] in (0xC0, 0xC2)][0]
    only_sof[sof[2] + 6] = G.PATCHED_ID
    hd = parse(bytes(only_sof), "convert")
    assert hd.kind == J.HOST and "component" in hd.reason


def test_four_components_go_to_the_host():
    cmyk = G.cmyk_jpeg()
    for fn in (J.parse, J.parse_progressive):
        hd = fn(cmyk, "convert")
        assert hd.kind == J.HOST and "4 components" in hd.reason, hd.reason
    out = io.BytesIO()
    Image.open(io.BytesIO(cmyk)).save(out, "JPEG", progressive=True)
    assert J.parse(out.getvalue(), "convert").kind == J.HOST
    hd = J.parse_progressive(out.getvalue(), "convert")
    assert hd.kind == J.HOST and "4 components" in hd.reason


def test_nothing_is_black_under_convert():
    files = [G.gray_file(k, s) for k in G.KINDS for s in G.SIZES] + [G.cmyk_jpeg(), G.png("L"), b"", b"\xff\xd8\xff"]
    for blob in files:
        assert J.parse(blob, "convert").kind in (J.DEVICE, J.HOST)
        assert J.parse_progressive(blob, "convert").kind in (J.DEVICE, J.HOST)


def test_truncated_gray_headers_never_raise():
    for kind in ("dri3", "progressive"):
        blob = G.gray_file(kind, (9, 17))
        for n in range(len(blob)):
            assert J.parse(blob[:n], "convert").kind in (J.DEVICE, J.HOST)
            assert J.parse_progressive(blob[:n], "convert").kind == J.HOST, n     # a cut file has no EOI


# ---------------------------------------------------------------------------------------------------------------
# batch plan
# ---------------------------------------------------------------------------------------------------------------
def test_header_record_keeps_its_size():
    assert J.HEADER_DTYPE.itemsize == 9016 and J.PROG_HEADER_DTYPE.itemsize == 432
    assert J.BLOCKS_PER_MCU[J.GRAY] == 1 and J.BLOCKS_PER_MCU[:3] == (3, 4, 6)


@pytest.mark.parametrize("scales", [[1, 1, 1, 1, 1], [2, 1, 4, 1, 2]], ids=["full", "drafted"])
def test_plan_of_a_batch_mixing_gray_and_colour(scales):
    gray = G.gray_file("dri3", SIZE)                                             # 5 x 7 blocks
    colour = encode(smooth_rgb(24, 40, seed=2), quality=90, subsampling=2)       # 40 x 24, 4:2:0: 3 x 2 MCUs of 6 blocks
    tiny = G.gray_file("baseline", (1, 1))
    pgray = G.gray_file("progressive", (9, 17))                                  # 2 x 3 blocks
    from test_jpeg_progressive_host import encode_progressive
    pcolour = encode_progressive(smooth_rgb(16, 16, seed=3), quality=90, subsampling=0)
    blobs, pblobs = [gray, colour, tiny], [pgray, pcolour]
    hdrs = [J.parse(b, "convert") for b in blobs]
    phdrs = [J.parse_progressive(b, "convert") for b in pblobs]
    assert [h.sampling for h in hdrs + phdrs] == [3, 2, 3, 3, 0]
    p = J.plan_device_batch([("base", hdrs, blobs), ("prog", phdrs, pblobs)], 2048, scales)
    rec = p.sections[0][1]
    prec = dict(p.sections)[p.prog_off[0]]
    assert rec.dtype == J.HEADER_DTYPE and prec.dtype == J.PROG_HEADER_DTYPE

    # blocks and planes: one plane of whole blocks for a gray image, 16-byte aligned slices
    blocks = [35, 36, 1]
    assert list(rec["coef_off"]) == [0, 35, 71] and p.tot["total_blocks"] == 72 and p.tot["max_blocks"] == 36
    planes = [(b * 64 + 15) // 16 * 16 for b in blocks]
    assert list(rec["plane_off"]) == [0, planes[0], planes[0] + planes[1]] and p.tot["total_plane_bytes"] == sum(planes)
    assert list(rec["sampling"]) == [3, 2, 3]
    assert [tuple(r) for r in rec[["mcus_x", "mcus_y"]].tolist()] == [(5, 7), (3, 2), (1, 1)]
    assert list(rec["restart"]) == [3, 6, 1] and list(rec["n_intervals"]) == [12, 1, 1]
    assert list(rec["int_off"]) == [0, 13, 15] and p.tot["total_intervals"] == 17 and p.tot["max_intervals"] == 12
    for r, h, blob in zip(rec, hdrs, blobs):
        scan = len(blob) - h.data_offset
        assert int(r["n_units"]) == -(-scan * 8 // 2048) + int(r["n_intervals"])
    assert list(prec["coef_off"]) == [0, 6] and p.ptot["total_blocks"] == 6 + 12 and p.coef_off == [0, 6, 18]
    assert list(prec["plane_off"]) == [0, 6 * 64] and list(prec["sampling"]) == [3, 0]
    assert [tuple(r) for r in prec[["mcus_x", "mcus_y"]].tolist()] == [(2, 3), (2, 2)]
    assert int(prec["n_intervals"][0]) == len(phdrs[0].scans)

    # tables: qt[0], DC slot 0, AC slot 3; the unused slots are zero
    for k in (0, 2):
        r = rec[k]
        assert np.array_equal(r["qt"][0], hdrs[k].qtables[0]) and not r["qt"][1:].any()
        for field in ("lut", "maxcode", "valoff", "huffval"):
            assert not r[field][[1, 2, 4, 5]].any(), field
        assert np.array_equal(r["lut"][0], J.device_tables(hdrs[k].dc_tables[0])[0])
        assert np.array_equal(r["lut"][3], J.device_tables(hdrs[k].ac_tables[0])[0])
        assert r["lut"][0].any() and r["lut"][3].any()
    assert rec[1]["qt"][2].any() and rec[1]["lut"][5].any()                      # the colour file keeps all of them
    assert not prec[0]["qt"][1:].any() and prec[1]["qt"][2].any()

    # scans of the gray progressive file: component 0 alone, its block raster
    srec = dict(p.sections)[p.prog_off[1]]
    mine = srec[srec["image"] == 0]
    assert len(mine) == len(phdrs[0].scans)
    assert set(mine["comp_mask"]) == {1} and set(mine["blocks_w"]) == {2} and set(mine["n_units"]) == {6}

    # output: H·W·3 bytes per image (or the drafted size), back to back, baseline first
    sizes = [J.scaled_size((h.width, h.height), s) for h, s in zip(hdrs + phdrs, scales)]
    nbytes = [w * h * 3 for w, h in sizes]
    assert p.out_offs == [int(x) for x in np.cumsum([0] + nbytes[:-1])]
    assert p.out_bytes == sum(nbytes[:3]) and p.pout_bytes == sum(nbytes[3:])
    assert list(rec["out_off"]) == p.out_offs[:3] and [p.out_bytes + int(o) for o in prec["out_off"]] == p.out_offs[3:]
    assert p.tot["max_width"] == max(s[0] for s in sizes[:3]) and p.tot["max_height"] == max(s[1] for s in sizes[:3])
    assert (p.scale_off is None) == (max(scales) == 1)


# ---------------------------------------------------------------------------------------------------------------
# host route
# ---------------------------------------------------------------------------------------------------------------
HOST_FILES = {
    "gray jpeg": lambda: G.gray_file("baseline", (64, 48)),
    "gray progressive jpeg": lambda: G.gray_file("progressive", (65, 47)),
    "cmyk jpeg": lambda: G.cmyk_jpeg(48, 64),
    "png L": lambda: G.png("L"),
    "png LA": lambda: G.png("LA"),
    "png P": lambda: G.png("P"),
    "png RGBA": lambda: G.png("RGBA"),
    "png I;16": lambda: G.png("I;16"),
}


@pytest.mark.parametrize("draft", [None, (16, 12), (8, 8), (5, 5)], ids=["full", "1/4", "1/4 again", "1/8"])
@pytest.mark.parametrize("name", HOST_FILES)
def test_host_route_converts(name, draft):
    blob = HOST_FILES[name]()
    mode = Image.open(io.BytesIO(blob)).mode
    assert mode != "RGB"
    want = G.pil_convert(blob, draft)
    got = DevicePreprocessor._pil_rgb(Image.open(io.BytesIO(blob)), draft, "convert")
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    if "jpeg" in name and draft is not None:
        assert got.shape[:2] != Image.open(io.BytesIO(blob)).size[::-1]          # the draft took
    if mode in ("L", "CMYK", "P", "RGBA"):
        assert want.any()                                                        # not a black canvas by accident
    pre = object.__new__(DevicePreprocessor)
    assert np.array_equal(pre._host_rgb(blob, draft, "convert"), want)
    # the default: zeros of the (drafted) size, with and without the keyword
    for black in (DevicePreprocessor._pil_rgb(Image.open(io.BytesIO(blob)), draft),
                  DevicePreprocessor._pil_rgb(Image.open(io.BytesIO(blob)), draft, "black"), pre._host_rgb(blob, draft)):
        assert black.shape == want.shape and black.dtype == np.uint8 and not black.any()


def test_host_route_leaves_rgb_files_alone():
    blob = encode(smooth_rgb(24, 40, seed=2), quality=90, subsampling=2)
    want = np.asarray(Image.open(io.BytesIO(blob)))
    for opt in ("black", "convert"):
        assert np.array_equal(DevicePreprocessor._pil_rgb(Image.open(io.BytesIO(blob)), None, opt), want)
