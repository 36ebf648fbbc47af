"""CPU side of the layouts="all" device JPEG route: what `jpeg.parse(f, layouts="all")` admits and refuses, that the default
stays what it was, the symbols (the HEADER_ANY_DTYPE record is checked in test_jpeg_cmyk_host), a numpy model
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


def test_abi_version_and_new_symbols():
    from on_device_image_captioning_amd import _hip
    from test_jpeg_cmyk_host import REMOVED
    lib = _hip.load()
    assert lib.odic_abi_version() == 27 == _hip.ABI_VERSION
    for name in ("odic_jpeg_any_workspace_bytes", "odic_jpeg_any_decode", "odic_jpeg_any_decode_scaled"):
        assert name in _hip.EXPORTED_SYMBOLS and getattr(lib, name).argtypes is not None
    assert lib.odic_jpeg_any_decode(None, None, 0, None) == -2
    assert lib.odic_jpeg_any_workspace_bytes(None) == 0
    raw = ctypes.CDLL(_hip.LIB_PATH)
    assert not any(name in _hip.EXPORTED_SYMBOLS or hasattr(raw, name) for name in REMOVED)


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
    plain = J.plan_device_batch([("base", hdrs, BASE)], 2048, [1])
    empty = J.plan_device_batch([("base", hdrs, BASE), ("prog", [], []), ("own", [], [])], 2048, [1])
    assert plain.group("own") is None and empty.group("own") is None and len(empty.groups) == 1
    assert [a.dtype for _, a in plain.sections] == [J.HEADER_DTYPE]
    host_a, host_b = np.zeros(plain.total, np.uint8), np.zeros(empty.total, np.uint8)
    plain.fill(host_a)
    empty.fill(host_b)
    assert plain.total == empty.total and np.array_equal(host_a, host_b) and plain.out_offs == empty.out_offs

    names = ["410-17x33", "440-7x9", "rgb-22-48x64"]
    lblobs = [L.CASES[n].blob for n in names]
    lhdrs = [J.parse(b, layouts="all") for b in lblobs]
    for base_h, base_b in ((hdrs, BASE), ([], [])):
        p = J.plan_device_batch([("base", base_h, base_b), ("own", lhdrs, lblobs)], 2048, [1] * len(base_h))
        g = p.group("own")
        assert (g.n, g.first) == (3, len(base_h))
        assert [a.dtype for _, a in p.sections] == [J.HEADER_DTYPE] * len(base_h) + [J.HEADER_ANY_DTYPE]
        spans = [(o, o + a.nbytes) for o, a in p.sections] + [(p.data_off, p.total)]
        assert all(lo % 256 == 0 for lo, _ in spans) and spans == sorted(spans)
        assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]))
        assert (p.sections[-1][0],) == g.offs
        host = np.full(p.total + 16, 0xA5, np.uint8)
        p.fill(host)
        assert (host[p.total:] == 0xA5).all()
        rec = host[g.offs[0]:g.offs[0] + 3 * J.HEADER_ANY_DTYPE.itemsize].view(J.HEADER_ANY_DTYPE)
        nb = len(base_h)
        for r, h, (o, _), blob in zip(rec, lhdrs, p.blobs[nb:], lblobs):
            lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
            assert (lo, hi) == (o + h.data_offset, o + len(blob)) and host[lo:hi].tobytes() == blob[h.data_offset:]
            assert list(zip(r["h"][:3], r["v"][:3])) == h.comp_hv and bool(r["color"]) == h.rgb and r["ncomp"] == 3
            assert (r["h"][3], r["v"][3]) == (0, 0) and not r["lut"][3].any() and not r["lut"][7].any()
            assert (int(r["mcus_x"]), int(r["mcus_y"])) == (h.mcus_x, h.mcus_y)
            assert int(r["out_off"]) % 4 == 0
        assert g.out_off % 256 == 0 and g.out_off >= p.out_bytes + p.pout_bytes
        assert p.out_offs[nb:] == [g.out_off + int(o) for o in rec["out_off"]]
        ends = [o + h.width * h.height * 3 for o, h in zip(p.out_offs[nb:], lhdrs)]
        assert all(e <= o for e, o in zip(ends, p.out_offs[nb + 1:])) and ends[-1] == g.out_off + g.out_bytes
        blocks = [h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv) for h in lhdrs]
        assert g.tot["total_blocks"] == sum(blocks) and g.tot["total_plane_bytes"] == 64 * sum(blocks)
        assert g.tot["max_blocks"] == max(blocks)


def test_batch_plan_holds_both_kinds_in_the_one_own_group():
    """A four-component and a `layout` file are one "own" group (they were two groups, the second placed behind the
    first): the first file's placement does not depend on the second, the two lie side by side in one record section and
    one stretch of the output, and the group's totals are the sums and maxima over both."""
    import jpeg_cmyk_cases as K
    cblobs = [K.CASES["cmyk-sub2-17x33"][0]]
    chdrs = [J.parse(b, "convert", cmyk="device", layouts="all") for b in cblobs]
    lblobs = [L.CASES["411-17x33"].blob]
    lhdrs = [J.parse(b, "convert", cmyk="device", layouts="all") for b in lblobs]
    hdrs = [J.parse(b) for b in BASE]
    only = J.plan_device_batch([("base", hdrs, BASE), ("own", chdrs, cblobs)], 2048, [1])
    p = J.plan_device_batch([("base", hdrs, BASE), ("own", chdrs + lhdrs, cblobs + lblobs)], 2048, [1])
    g, og = p.group("own"), only.group("own")
    assert [a.dtype for _, a in p.sections] == [J.HEADER_DTYPE, J.HEADER_ANY_DTYPE] and [x.kind for x in p.groups] == ["base", "own"]
    assert (g.offs, g.out_off, g.first, p.out_offs[:2]) == (og.offs, og.out_off, og.first, only.out_offs)
    assert g.offs[0] % 256 == 0 and g.out_off == J.pad256(p.out_bytes) and (g.n, og.n) == (2, 1)
    # the second image behind the first, on a whole word, inside the group's bytes; nothing overlaps
    assert p.out_offs[2] == g.out_off + (og.out_bytes + 3) // 4 * 4 and p.out_offs[2] % 4 == 0
    assert p.out_offs[2] >= p.out_offs[1] + chdrs[0].width * chdrs[0].height * 3
    assert p.out_offs[2] + lhdrs[0].width * lhdrs[0].height * 3 == g.out_off + g.out_bytes
    host = np.zeros(p.total, np.uint8)
    p.fill(host)
    rec = host[g.offs[0]:g.offs[0] + 2 * J.HEADER_ANY_DTYPE.itemsize].view(J.HEADER_ANY_DTYPE)
    assert g.offs[0] + rec.nbytes <= p.data_off and list(rec["ncomp"]) == [4, 3]
    spans = []
    for r, h, blob in zip(rec, chdrs + lhdrs, cblobs + lblobs):
        lo, hi = p.data_off + int(r["data_off"]), p.data_off + int(r["data_end"])
        assert host[lo:hi].tobytes() == blob[h.data_offset:]
        assert list(zip(r["h"][:h.ncomp], r["v"][:h.ncomp])) == h.comp_hv
        spans.append((lo, hi))
    assert spans[0][1] <= spans[1][0] and spans[1][1] == p.total
    # coefficient blocks and planes of the second image start where the first one's end
    blocks = [h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv) for h in chdrs + lhdrs]
    assert list(rec["coef_off"]) == [0, blocks[0]] and list(rec["plane_off"]) == [0, 64 * blocks[0]]
    assert g.tot["total_blocks"] == sum(blocks) == og.tot["total_blocks"] + blocks[1]
    assert g.tot["total_plane_bytes"] == 64 * sum(blocks) and g.tot["max_blocks"] == max(blocks)
    assert g.tot["max_width"] == max(h.width for h in chdrs + lhdrs)
    assert g.tot["max_height"] == max(h.height for h in chdrs + lhdrs)
