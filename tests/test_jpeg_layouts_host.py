"""CPU side of the layouts="all" device JPEG route: what `jpeg.parse(f, layouts="all")` admits and refuses, that the default
stays what it was, the HEADER3_DTYPE record against a ctypes mirror of odic_jpeg_header3, the new symbols, a numpy model
of the whole tail (IDCT planes from the writer's coefficients, libjpeg's upsampling rule per component, colour) against
Pillow on every case, and the batch plan's extra group."""
import ctypes
import io

import numpy as np
import pytest
from PIL import Image

from on_device_image_captioning_amd import jpeg as J

import jpeg_layout_cases as L
from test_jpeg_host import encode, model_idct, smooth_rgb


def same(a, b):
    """Two headers field for field (the quantisation tables are arrays)."""
    da, db = dict(vars(a)), dict(vars(b))
    qa, qb = da.pop("qtables"), db.pop("qtables")
    return da == db and len(qa) == len(qb) and all(np.array_equal(x, y) for x, y in zip(qa, qb))


@pytest.mark.parametrize("name", L.CASES)
def test_default_parse_is_unchanged(name):
    c = L.CASES[name]
    h = J.parse(c.blob)
    want = "not YCbCr" if c.rgb or c.style == "bareXYZ" else f"sampling {c.hv}"
    assert (h.kind, h.reason) == (J.HOST, want)
    assert J.parse(c.blob, layouts="common") == h and J.parse(c.blob, "convert") == h
    assert J.parse_progressive(c.blob).kind == J.HOST


@pytest.mark.parametrize("name", L.CASES)
def test_admitted_cases_parse_as_device(name):
    c = L.CASES[name]
    with Image.open(io.BytesIO(c.blob)) as im:
        assert im.mode == "RGB" and im.size == c.size
    h = J.parse(c.blob, layouts="all")
    assert h.kind == J.DEVICE, h.reason
    assert h.ncomp == 3 and h.layout and h.comp_hv == c.hv and h.rgb is c.rgb and h.sampling == -1
    assert (h.width, h.height) == c.size
    mw, mh = L.mcu_size(c.hv)
    assert (h.mcus_x, h.mcus_y) == (-(-h.width // mw), -(-h.height // mh)) == c.mcus
    assert len(h.qtables) == 3 and len(h.dc_tables) == 3 and len(h.ac_tables) == 3
    assert h.restart_interval == c.restart
    assert same(J.parse(c.blob, "convert", cmyk="device", layouts="all"), h)


@pytest.mark.parametrize("name", L.refused())
def test_refused_cases_go_to_the_host_with_a_reason(name):
    blob, word, kw = L.refused()[name]
    h = J.parse(blob, **kw)
    assert h.kind == J.HOST and word in h.reason, h.reason
    assert h.reason != "SOF2"                              # that reason sends a file to parse_progressive


def test_common_files_parse_as_they_do_without_the_keyword():
    for sub in (0, 1, 2):
        for kw in (dict(), dict(progressive=True)):
            f = encode(smooth_rgb(24, 40, seed=sub), quality=90, subsampling=sub, **kw)
            a, b = J.parse(f, layouts="all"), J.parse(f)
            assert same(a, b) and not a.layout and (a.kind == J.DEVICE) == (not kw) and (b.reason == "SOF2") == bool(kw)
    gray = encode(smooth_rgb(16, 16, seed=3).mean(axis=2).astype(np.uint8), quality=90)
    for non_rgb in J.NON_RGB:
        assert same(J.parse(gray, non_rgb, layouts="all"), J.parse(gray, non_rgb))


def test_check_layouts():
    assert J.check_layouts("common") == "common" and J.check_layouts("all") == "all"
    for bad in ("every", "", None, True, "ALL"):
        with pytest.raises(ValueError, match="layouts"):
            J.check_layouts(bad)
        with pytest.raises(ValueError, match="layouts"):
            J.parse(L.CASES["440-7x9"].blob, layouts=bad)


class Header3(ctypes.Structure):
    """odic_jpeg_header3 as include/odic_hip.h declares it."""
    _fields_ = [(n, ctypes.c_int64) for n in ("data_off", "data_end", "out_off", "scan_off", "coef_off", "plane_off")] + \
               [(n, ctypes.c_int32) for n in ("int_off", "unit_off", "width", "height", "rgb", "mcus_x", "mcus_y", "restart",
                                             "n_intervals", "n_units")] + \
               [("h", ctypes.c_int32 * 3), ("v", ctypes.c_int32 * 3), ("qt", ctypes.c_uint16 * 64 * 3),
                ("lut", ctypes.c_uint16 * 512 * 6), ("maxcode", ctypes.c_int32 * 18 * 6), ("valoff", ctypes.c_int32 * 18 * 6),
                ("huffval", ctypes.c_uint8 * 256 * 6)]


def test_header3_record_matches_the_c_struct():
    assert J.HEADER3_DTYPE.itemsize == ctypes.sizeof(Header3) == 9040      # the static_assert in csrc/jpeg_decode.hip
    assert list(J.HEADER3_DTYPE.names) == [n for n, _ in Header3._fields_]
    for name, _ in Header3._fields_:
        dt, off = J.HEADER3_DTYPE.fields[name][:2]
        f = getattr(Header3, name)
        assert (off, dt.itemsize) == (f.offset, f.size), name
    for name in J.HEADER_DTYPE.names[:10]:                 # the common prefix the templated kernels read
        assert J.HEADER3_DTYPE.fields[name][1] == J.HEADER_DTYPE.fields[name][1]
    for name in ("mcus_x", "mcus_y", "restart", "n_intervals", "n_units", "h"):
        assert J.HEADER3_DTYPE.fields[name][1] == J.HEADER4_DTYPE.fields[name][1]
    assert J.HEADER_DTYPE.itemsize == 9016 and J.HEADER4_DTYPE.itemsize == 12024


def test_abi_version_and_new_symbols():
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    assert lib.odic_abi_version() == 26 == _hip.ABI_VERSION
    for name in ("odic_jpeg3_any_workspace_bytes", "odic_jpeg3_any_decode"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.odic_jpeg3_any_decode(None, None, 0, None) == -2
    assert lib.odic_jpeg3_any_workspace_bytes(None) == 0


# ------------------------------------------------------------------------------------------------------------
# the tail after the entropy decode, in numpy
# ------------------------------------------------------------------------------------------------------------
def model_planes(c):
    """jidctint.c on the writer's coefficients → the three planes, mcus_x·8·h wide and mcus_y·8·v high."""
    mx, my = c.mcus
    q = np.full(64, c.q, np.int64)
    planes = []
    for coef, (h, v) in zip(c.coefs, c.hv):
        pix = model_idct(coef.reshape(-1, 64), q).reshape(my, mx, v, h, 8, 8)
        planes.append(pix.transpose(0, 2, 4, 1, 3, 5).reshape(my * v * 8, mx * h * 8))
    return planes


def model_upsample(P, rh, rv, dw, dh, W, H):
    """jdsample.c: one plane with 1 / rh of the output's width and 1 / rv of its height → int64 [H, W].  dw, dh: the
    plane's real samples (the clamp at the edges)."""
    P = P.astype(np.int64)
    x, y = np.arange(W), np.arange(H)
    if (rh, rv) == (1, 2):                                 # h1v2_fancy_upsample, at every width
        r = y >> 1
        rn = np.where(y & 1, np.minimum(r + 1, dh - 1), np.maximum(r - 1, 0))
        return (3 * P[r][:, x] + P[rn][:, x] + np.where(y & 1, 2, 1)[:, None]) >> 2
    if (rh, rv) in ((2, 1), (2, 2)) and dw > 2:
        c = x >> 1
        cn = np.where(x & 1, np.minimum(c + 1, dw - 1), np.maximum(c - 1, 0))
        if rv == 1:                                        # h2v1_fancy_upsample
            return (3 * P[y][:, c] + P[y][:, cn] + np.where(x & 1, 2, 1)) >> 2
        r = y >> 1                                         # h2v2_fancy_upsample
        rn = np.where(y & 1, np.minimum(r + 1, dh - 1), np.maximum(r - 1, 0))
        cs = 3 * P[r] + P[rn]
        return (3 * cs[:, c] + cs[:, cn] + np.where(x & 1, 7, 8)) >> 4
    return P[y // rv][:, x // rh]                          # fullsize, h2v1 / h2v2_upsample, int_upsample: replication


def model_rgb(c):
    W, H = c.size
    hmax, vmax = max(h for h, _ in c.hv), max(v for _, v in c.hv)
    s = [model_upsample(P, hmax // h, vmax // v, -(-W * h // hmax), -(-H * v // vmax), W, H)
         for P, (h, v) in zip(model_planes(c), c.hv)]
    if not c.rgb:                                          # jdcolor.c ycc_rgb_convert
        yy, cb, cr = s[0], s[1] - 128, s[2] - 128
        s = [yy + ((91881 * cr + 32768) >> 16), yy + ((-22554 * cb - 46802 * cr + 32768) >> 16),
             yy + ((116130 * cb + 32768) >> 16)]
    return np.clip(np.stack(s, axis=2), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("name", L.CASES)
def test_model_of_the_tail_is_pillows_decode(name):
    c = L.CASES[name]
    want = L.oracle(c.blob)
    got = model_rgb(c)
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, (len(bad), bad[:8].tolist())


def test_the_width_rule_holds_for_h2v1_and_h2v2_only():
    """At 3x5 every sub-sampled plane is at most two samples wide: h2v1 / h2v2 replicate there, h1v2 still filters."""
    c = L.CASES["440-3x5"]
    P = model_planes(c)[1]
    assert not np.array_equal(model_upsample(P, 1, 2, 3, 3, 3, 5), P.astype(np.int64)[np.arange(5) // 2][:, :3])


BASE = [encode(smooth_rgb(16, 16, seed=1), quality=90, subsampling=0)]


def test_batch_plan_lists_the_group_only_when_a_file_is_there():
    hdrs = [J.parse(b, layouts="all") for b in BASE]
    assert all(same(a, J.parse(b)) for a, b in zip(hdrs, BASE))
    plain = J.plan_device_batch(hdrs, BASE, [], [], 2048, [1])
    empty = J.plan_device_batch(hdrs, BASE, [], [], 2048, [1], [], [], [], [])
    assert plain.ltot is None and plain.layout_off is None and plain.lout_bytes == 0
    assert [a.dtype for _, a in plain.sections] == [J.HEADER_DTYPE]
    host_a, host_b = np.zeros(plain.total, np.uint8), np.zeros(empty.total, np.uint8)
    plain.fill(host_a)
    empty.fill(host_b)
    assert plain.total == empty.total and np.array_equal(host_a, host_b) and plain.out_offs == empty.out_offs

    names = ["410-17x33", "440-7x9", "rgb-22-48x64"]
    lblobs = [L.CASES[n].blob for n in names]
    lhdrs = [J.parse(b, layouts="all") for b in lblobs]
    for base_h, base_b in ((hdrs, BASE), ([], [])):
        p = J.plan_device_batch(base_h, base_b, [], [], 2048, [1] * len(base_h), [], [], lhdrs, lblobs)
        assert [a.dtype for _, a in p.sections] == [J.HEADER_DTYPE] * len(base_h) + [J.HEADER3_DTYPE]
        spans = [(o, o + a.nbytes) for o, a in p.sections] + [(p.data_off, p.total)]
        assert all(lo % 256 == 0 for lo, _ in spans) and spans == sorted(spans)
        assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]))
        assert p.sections[-1][0] == p.layout_off and p.cmyk_off is None
        host = np.full(p.total + 16, 0xA5, np.uint8)
        p.fill(host)
        assert (host[p.total:] == 0xA5).all()
        rec = host[p.layout_off:p.layout_off + 3 * J.HEADER3_DTYPE.itemsize].view(J.HEADER3_DTYPE)
        nb = len(base_h)
        for r, h, (o, _), blob in zip(rec, lhdrs, p.blobs[nb:], lblobs):
            lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
            assert (lo, hi) == (o + h.data_offset, o + len(blob)) and host[lo:hi].tobytes() == blob[h.data_offset:]
            assert list(zip(r["h"], r["v"])) == h.comp_hv and bool(r["rgb"]) == h.rgb
            assert (int(r["mcus_x"]), int(r["mcus_y"])) == (h.mcus_x, h.mcus_y)
            assert int(r["out_off"]) % 4 == 0
        assert p.lout_off % 256 == 0 and p.lout_off >= p.out_bytes + p.pout_bytes
        assert p.out_offs[nb:] == [p.lout_off + int(o) for o in rec["out_off"]]
        ends = [o + h.width * h.height * 3 for o, h in zip(p.out_offs[nb:], lhdrs)]
        assert all(e <= o for e, o in zip(ends, p.out_offs[nb + 1:])) and ends[-1] == p.lout_off + p.lout_bytes
        blocks = [h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv) for h in lhdrs]
        assert p.ltot["total_blocks"] == sum(blocks) and p.ltot["total_plane_bytes"] == 64 * sum(blocks)
        assert p.ltot["max_blocks"] == max(blocks)


def test_batch_plan_places_the_group_behind_the_four_component_one():
    import jpeg_cmyk_cases as K
    cblobs = [K.CASES["cmyk-sub2-17x33"][0]]
    chdrs = [J.parse(b, "convert", cmyk="device", layouts="all") for b in cblobs]
    lblobs = [L.CASES["411-17x33"].blob]
    lhdrs = [J.parse(b, "convert", cmyk="device", layouts="all") for b in lblobs]
    hdrs = [J.parse(b) for b in BASE]
    only = J.plan_device_batch(hdrs, BASE, [], [], 2048, [1], chdrs, cblobs)
    p = J.plan_device_batch(hdrs, BASE, [], [], 2048, [1], chdrs, cblobs, lhdrs, lblobs)
    assert [a.dtype for _, a in p.sections] == [J.HEADER_DTYPE, J.HEADER4_DTYPE, J.HEADER3_DTYPE]
    assert (p.cmyk_off, p.cout_off, p.cout_bytes, p.out_offs[:2]) == (only.cmyk_off, only.cout_off, only.cout_bytes,
                                                                      only.out_offs)
    assert p.layout_off == p.cmyk_off + J.pad256(J.HEADER4_DTYPE.itemsize)
    assert p.lout_off == J.pad256(p.cout_off + p.cout_bytes) and p.out_offs[2] == p.lout_off
    host = np.zeros(p.total, np.uint8)
    p.fill(host)
    c4 = host[p.cmyk_off:p.cmyk_off + J.HEADER4_DTYPE.itemsize].view(J.HEADER4_DTYPE)[0]
    l3 = host[p.layout_off:p.layout_off + J.HEADER3_DTYPE.itemsize].view(J.HEADER3_DTYPE)[0]
    for r, h, blob in ((c4, chdrs[0], cblobs[0]), (l3, lhdrs[0], lblobs[0])):
        lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
        assert host[lo:hi].tobytes() == blob[h.data_offset:]
