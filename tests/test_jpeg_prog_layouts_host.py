"""CPU side of the progressive per-component-sampling routes: the case files of jpeg_prog_layout_cases.py against Pillow
(the new writer is checked against Pillow alone), `jpeg.parse_progressive` with cmyk="device" / layouts="all" and with
the defaults, the refused set, the packed records, the batch plan with the new group, and the binding."""
import ctypes
import io
import warnings

import numpy as np
import pytest
from PIL import Image

import jpeg_prog_layout_cases as P
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb
from test_jpeg_progressive_host import CScan, encode_progressive

WRITER_CASES = [n for n, c in P.CASES.items() if isinstance(c, P.Case)]


def test_the_case_list_covers_what_it_should():
    assert len(P.CASES) == len(WRITER_CASES) + 9 and len(WRITER_CASES) == 12 * 7 + 5 * 5
    sizes = {c.size for c in P.CASES.values()}
    assert {(1, 1), (3, 5), (7, 9), (17, 33), (48, 64)} <= sizes
    assert sum(J.MAX_MCU_BLOCKS == sum(h * v for h, v in c.hv) for c in P.CASES.values()) >= 2 * 7      # 4:1:0, Photoshop


@pytest.mark.parametrize("name", P.CASES)
def test_case_file_opens_in_pillow_without_a_warning(name):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(P.CASES[name].blob))
        assert im.size == P.CASES[name].size and im.mode == ("CMYK" if P.CASES[name].ncomp == 4 else "RGB")
        im.load()


@pytest.mark.parametrize("name", WRITER_CASES)
def test_progressive_file_decodes_as_its_baseline_twin(name):
    """The scans of the new writer carry exactly the coefficients the baseline writers code: Pillow says so."""
    c = P.CASES[name]
    assert np.array_equal(P.oracle(c.blob), P.oracle(c.baseline()))


@pytest.mark.parametrize("name", P.CASES)
def test_parse_progressive_admits_the_case(name):
    c = P.CASES[name]
    hd = J.parse_progressive(c.blob, **P.KW[c.ncomp])
    assert hd.kind == J.DEVICE, hd.reason
    assert (hd.width, hd.height) == c.size and hd.ncomp == c.ncomp and hd.comp_hv == list(c.hv)
    assert (hd.ycck if c.ncomp == 4 else hd.rgb) == c.color and hd.layout == (c.ncomp == 3)
    mw, mh = 8 * max(h for h, _ in c.hv), 8 * max(v for _, v in c.hv)
    assert (hd.mcus_x, hd.mcus_y) == (-(-c.size[0] // mw), -(-c.size[1] // mh))
    if c.script is None:
        return
    assert len(hd.scans) == len(c.script)
    for got, sc in zip(hd.scans, c.script):
        assert (tuple(got.comps), got.ss, got.se, got.ah, got.al) == (tuple(sc.comps), sc.ss, sc.se, sc.ah, sc.al)
        assert (got.n_units, got.blocks_w) == P.expected_scan(c, sc)
        assert got.restart_interval == sc.restart
    # DC first → (DC refinement | first AC pass) → each AC refinement: an AC scan waits for its component's first DC scan
    # only, so the whole-band AC scans of the two DC scripts share the DC refinement's level
    levels = {"separate-dc": 2, "partial-dc": 2, "split-refine": 4}
    kind = next((k for k in levels if name.endswith(k)), None)
    assert hd.n_levels == (levels[kind] if kind else 3 if "dri" in name else 4)


@pytest.mark.parametrize("name", P.CASES)
def test_default_keywords_keep_the_case_on_the_host(name):
    """Without the opt-ins both parsers say what they said before the route existed."""
    c = P.CASES[name]
    if c.ncomp == 4:
        assert J.parse_progressive(c.blob).kind == J.BLACK
        hd = J.parse_progressive(c.blob, "convert")
        assert (hd.kind, hd.reason) == (J.HOST, "4 components (CMYK / YCCK)")
        assert J.parse(c.blob, "convert", cmyk="device").reason == J.PROG_CMYK_REASON
        assert J.parse_progressive(c.blob, "convert", layouts="all").reason == "4 components (CMYK / YCCK)"
    else:
        hd = J.parse_progressive(c.blob)
        assert hd.kind == J.HOST and hd.reason == ("not YCbCr" if c.color else f"sampling {list(c.hv)}")
        assert J.parse(c.blob, layouts="all").reason == f"{J.PROG_LAYOUT_REASON}: {list(c.hv)}"
        assert J.parse(c.blob).reason == "SOF2"


def test_common_files_parse_as_without_the_keywords():
    for sub in (0, 1, 2):
        f = encode_progressive(smooth_rgb(24, 40, seed=sub), quality=90, subsampling=sub)
        a, b = J.parse_progressive(f, "convert", cmyk="device", layouts="all"), J.parse_progressive(f)
        assert a.kind == J.DEVICE and not a.layout and repr(a) == repr(b)
    base = encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=0)
    assert J.parse_progressive(base, layouts="all").reason == J.parse_progressive(base).reason == "SOF0"
    with pytest.raises(ValueError, match="non_rgb='convert'"):
        J.parse_progressive(base, cmyk="device")


@pytest.mark.parametrize("name", P.refused())
def test_refused_files_come_back_with_their_reason(name):
    blob, word, kw = P.refused()[name]
    hd = J.parse_progressive(blob, **kw)
    assert hd.kind == J.HOST and word in hd.reason, hd.reason


class CProgHeaderAny(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int64) for n in ("out_off", "coef_off", "plane_off")] + \
               [(n, ctypes.c_int32) for n in ("width", "height", "color", "mcus_x", "mcus_y", "n_intervals", "ncomp",
                                              "pad")] + \
               [("h", ctypes.c_int32 * 4), ("v", ctypes.c_int32 * 4), ("qt", ctypes.c_uint16 * 64 * 4)]


def test_record_matches_the_c_struct():
    """The same declaration as include/odic_hip.h (whose size and offsets csrc/jpeg_decode.hip static_asserts)."""
    dt = J.PROG_HEADER_ANY_DTYPE
    assert dt.itemsize == ctypes.sizeof(CProgHeaderAny) == 600
    assert list(dt.names) == [f[0] for f in CProgHeaderAny._fields_]
    for name in dt.names:
        assert dt.fields[name][1] == getattr(CProgHeaderAny, name).offset, name
    for name in ("out_off", "coef_off", "plane_off", "width", "height", "mcus_x", "mcus_y", "n_intervals"):
        assert dt.fields[name][1] == J.PROG_HEADER_DTYPE.fields[name][1], name               # the common prefix
    assert dt.fields["color"][1] == J.PROG_HEADER_DTYPE.fields["sampling"][1]
    assert J.SCAN_DTYPE.itemsize == ctypes.sizeof(CScan) == 88 and J.SCAN_DTYPE.fields["pad"][1] == 84


NEW = ["photoshop-17x33", "440-dri3", "c4-11-7x9", "11-21-21-partial-dc"]


def new_group():
    blobs = [P.CASES[n].blob for n in NEW]
    hdrs = [J.parse_progressive(b, **P.KW[P.CASES[n].ncomp]) for n, b in zip(NEW, blobs)]
    assert all(h.kind == J.DEVICE for h in hdrs)
    return hdrs, blobs


def test_packed_records_describe_the_batch():
    hdrs, blobs = new_group()
    offs = [0, 5000, 9000, 20000]
    rec, srec, trec, tot, out_offs, out_bytes = J.pack_progressive(hdrs, offs, dtype=J.PROG_HEADER_ANY_DTYPE)
    assert rec.dtype == J.PROG_HEADER_ANY_DTYPE and len(rec) == 4 and len(srec) == sum(len(h.scans) for h in hdrs)
    assert list(rec["ncomp"]) == [4, 3, 4, 3] and list(rec["color"]) == [1, 0, 0, 0]
    assert rec["h"].tolist() == [[2, 1, 1, 2], [1, 1, 1, 0], [1, 1, 1, 1], [1, 2, 2, 0]]
    assert rec["v"].tolist() == [[2, 1, 1, 2], [2, 1, 1, 0], [1, 1, 1, 1], [1, 1, 1, 0]]
    assert all(o % 4 == 0 for o in out_offs) and out_bytes >= sum(h.width * h.height * 3 for h in hdrs)
    blocks = [h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv) for h in hdrs]
    assert list(rec["coef_off"]) == list(np.cumsum([0] + blocks[:-1])) and tot["total_blocks"] == sum(blocks)
    assert tot["total_plane_bytes"] == 64 * sum(blocks) and tot["max_blocks"] == max(blocks)
    for k, h in enumerate(hdrs):
        mine = srec[srec["image"] == k]
        assert rec[k]["n_intervals"] == mine["n_intervals"].sum() == sum(s.n_intervals for s in h.scans)
        assert sorted(mine["data_off"] - offs[k]) == sorted(s.data_offset for s in h.scans)
        assert (mine["comp_mask"] < (1 << h.ncomp)).all()
    # the interleaved first DC scan of four components names four tables, the fourth in the spare word; no other scan
    # touches that word
    dc4 = srec[(srec["comp_mask"] == 15) & (srec["ah"] == 0)]
    assert len(dc4) == 2 and (dc4["table"] >= 0).all() and (dc4["pad"] >= 0).all() and (dc4["pad"] < tot["n_tables"]).all()
    rest = srec[~((srec["comp_mask"] == 15) & (srec["ah"] == 0))]
    assert (rest["pad"] == -1).all() and (srec["table"] < tot["n_tables"]).all()
    # the existing record keeps its spare word at zero
    old = J.pack_progressive([J.parse_progressive(encode_progressive(smooth_rgb(16, 16, seed=3), quality=90))], [0])
    assert old[0].dtype == J.PROG_HEADER_DTYPE and (old[1]["pad"] == 0).all()


BASE = [encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=0)]
PROG = [encode_progressive(smooth_rgb(16, 16, seed=3), quality=90, subsampling=0)]


def filled(p):
    host = np.full(p.total + 64, 0xA5, np.uint8)
    p.fill(host)
    return host


def test_plan_without_the_new_files_is_unchanged():
    hdrs, phdrs = [J.parse(b) for b in BASE], [J.parse_progressive(b) for b in PROG]
    a = J.plan_device_batch([("base", hdrs, BASE), ("prog", phdrs, PROG)], 2048, [1, 1])
    b = J.plan_device_batch([("base", hdrs, BASE), ("prog", phdrs, PROG), ("pany", [], [])], 2048, [1, 1])
    assert a.group("pany") is None and b.group("pany") is None and [g.kind for g in b.groups] == ["base", "prog"]
    assert a.total == b.total and a.out_offs == b.out_offs and np.array_equal(filled(a), filled(b))
    assert [o for o, _ in a.sections] == [o for o, _ in b.sections] and len(a.sections) == 4


def test_plan_with_the_new_group():
    ahdrs, ablobs = new_group()
    hdrs, phdrs = [J.parse(b) for b in BASE], [J.parse_progressive(b) for b in PROG]
    lay = P.CASES["440-17x33"].baseline()
    lhdrs = [J.parse(lay, layouts="all")]
    three = [("base", hdrs, BASE), ("prog", phdrs, PROG), ("own", lhdrs, [lay])]
    without = J.plan_device_batch(three, 2048, [1, 1])
    p = J.plan_device_batch(three + [("pany", ahdrs, ablobs)], 2048, [1, 1])
    own, pany = p.group("own"), p.group("pany")
    # the other groups' records lie where they lay, and their output too; the new records follow the others'
    assert [o for o, _ in p.sections[:len(without.sections)]] == [o for o, _ in without.sections]
    assert p.out_offs[:3] == without.out_offs and own.out_off == without.group("own").out_off
    assert [a.dtype for _, a in p.sections[-3:]] == [J.PROG_HEADER_ANY_DTYPE, J.SCAN_DTYPE, J.TABLE_DTYPE]
    assert list(pany.offs) == [o for o, _ in p.sections[-3:]] and pany.offs[0] >= without.data_off
    spans = [(o, o + a.nbytes) for o, a in p.sections] + [(p.data_off, p.total)]
    assert all(lo % 256 == 0 for lo, _ in spans) and spans == sorted(spans)
    assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]))
    # files verbatim, the new ones last; every scan record points into its own file
    host = filled(p)
    assert (host[p.total:] == 0xA5).all() and len(p.blobs) == 3 + len(ablobs)
    for (o, a), blob in zip(p.blobs[3:], ablobs):
        assert host[o:o + len(blob)].tobytes() == blob
    srec = dict(p.sections)[pany.offs[1]]
    for r in srec:
        o, blob = p.blobs[3 + int(r["image"])][0], ablobs[int(r["image"])]
        assert o <= p.data_off + int(r["data_off"]) <= p.data_off + int(r["data_end"]) <= o + len(blob)
    # output: behind the layout group from the next multiple of 256, images disjoint
    assert pany.out_off == J.pad256(own.out_off + own.out_bytes) and pany.out_off % 256 == 0
    mine = p.out_offs[3:]
    sizes = [h.width * h.height * 3 for h in ahdrs]
    assert mine[0] == pany.out_off and all(a + n <= b for a, n, b in zip(mine, sizes, mine[1:]))
    assert mine[-1] + sizes[-1] == pany.out_off + pany.out_bytes
    assert [pany.out_off + int(o) for o in dict(p.sections)[pany.offs[0]]["out_off"]] == mine


def test_binding_and_abi():
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    assert _hip.ABI_VERSION == 27 == lib.odic_abi_version()
    for name in ("odic_jpeg_progressive_any_workspace_bytes", "odic_jpeg_decode_progressive_any"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name)
    assert lib.odic_jpeg_decode_progressive_any(None, None, 0, None) == -2
    assert lib.odic_jpeg_progressive_any_workspace_bytes(None) == 0
    header = open(_hip.LIB_PATH.replace("on_device_image_captioning_amd/libodic_hip.so", "include/odic_hip.h")).read()
    assert "odic_jpeg_decode_progressive_any(const odic_jpeg_prog_batch* batch" in header
