"""CPU side of the draft-scale decode of JPEGs with per-component sampling (draft_layouts="all"): libjpeg's
per-component transform sizes (`jpeg.scaled_components`) proven against Pillow by a numpy model of the scaled decode,
the three record packers with scales, and the `draft_layouts` keyword through the parser and plan functions."""
import ctypes
import os

import numpy as np
import pytest

import jpeg_draft_layout_model as M
import test_jpeg_host as H
from on_device_image_captioning_amd import jpeg as J


# ------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------
def test_scaled_components_on_known_layouts():
    sc = J.scaled_components
    c420, c422, c411 = [(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(4, 1), (1, 1), (1, 1)]
    assert sc(c420, 1) == [(8, 1, 1), (8, 2, 2), (8, 2, 2)]
    assert sc(c420, 2) == [(4, 1, 1), (8, 1, 1), (8, 1, 1)]              # 4:2:0 chroma doubles: no upsampling left
    assert sc(c420, 8) == [(1, 1, 1), (2, 1, 1), (2, 1, 1)]
    assert sc(c422, 2) == [(4, 1, 1), (4, 2, 1), (4, 2, 1)]              # 4:2:2 chroma stays: h2v1
    assert [sc(c411, s)[1] for s in (2, 4, 8)] == [(4, 4, 1), (2, 4, 1), (1, 4, 1)]      # 4:1:1 chroma never doubles
    assert sc([(4, 2), (1, 1), (1, 1)], 2)[1] == (8, 2, 1)               # 4:1:0: doubles once, h2v1 remains
    assert sc([(1, 2), (1, 1), (1, 1)], 4) == [(2, 1, 1), (2, 1, 2), (2, 1, 2)]          # 4:4:0: h1v2
    assert sc([(1, 1), (2, 1), (2, 1)], 2) == [(4, 2, 1), (4, 1, 1), (4, 1, 1)]          # component 0 upsampled
    assert sc(M.PHOTOSHOP_HV, 2) == [(4, 1, 1), (8, 1, 1), (8, 1, 1), (4, 1, 1)]
    for hv, _ in M.LAYOUTS.values():
        assert sc(hv, 1) == [(8, max(a for a, _ in hv) // h, max(b for _, b in hv) // v) for h, v in hv]
        for s in (2, 4, 8):
            for (h, v), (n, rh, rv) in zip(hv, sc(hv, s)):
                assert n in (1, 2, 4, 8) and n >= 8 // s and rh >= 1 and rv >= 1
                # the output grid: every component covers the same area
                assert n * h * rh == (8 // s) * max(a for a, _ in hv) and n * v * rv == (8 // s) * max(b for _, b in hv)
    with pytest.raises(ValueError):
        sc(c420, 3)


@pytest.mark.parametrize("layout", M.LAYOUTS)
def test_numpy_model_of_the_scaled_decode_is_bit_exact_with_pillow(layout):
    """What pins `scaled_components`, the downsampled sizes and the fancy / plain switch against the Pillow of this
    machine: baseline and progressive files from the same coefficients, at every scale a request can reach."""
    reached = set()
    for name, case in M.CASES.items():
        if case.layout != layout:
            continue
        files = [case.baseline(), case.progressive()]
        for s in M.SCALES:
            req = M.request_for(case.size, s)
            if J.draft_scale(case.size, req) != s:        # an image 3 pixels across cannot be asked for 1/4
                continue
            got = M.model_draft_rgb(case, s)
            for f in files:
                want, chosen = M.pil_draft_rgb(f, req)
                assert chosen == s
                assert got.shape == want.shape and np.array_equal(got, want), (name, s)
            reached.add((case.size, s))
    assert {s for _, s in reached} == set(M.SCALES)
    assert ((3, 40), 2) in reached and ((40, 3), 2) in reached and ((9, 36), 4) in reached


def test_the_narrow_cases_take_the_plain_path():
    """3 x 40 at 1/2 and 9 x 36 at 1/4: a plane that is upsampled 2:1 across has at most two real samples."""
    hit = 0
    for (w, h), s in (((3, 40), 2), ((9, 36), 4)):
        for hv, _ in M.LAYOUTS.values():
            hmax = max(a for a, _ in hv)
            for (a, _), (n, rh, rv) in zip(hv, J.scaled_components(hv, s)):
                if rh == 2 and rv == 1:
                    assert -(-w * a * n // (hmax * 8)) <= 2
                    hit += 1
    assert hit >= 8


# ------------------------------------------------------------------------------------------------------------
# packing
# ------------------------------------------------------------------------------------------------------------
PACK = [("440-93x67", 2), ("410-48x64", 8), ("22-21-21-17x33", 1), ("11-21-21-93x67", 4), ("rgb-22-48x64", 2)]
PACK4 = [("photoshop-ycck-93x67", 2), ("cmyk-21-48x64", 4), ("cmyk-11-17x33", 1), ("ycck-22-93x67", 8)]


def _check_records(rec, tot, out_offs, out_bytes, hdrs, scales):
    pos = planes = 0
    for r, h, s, off in zip(rec, hdrs, scales, out_offs):
        w, hh = J.scaled_size((h.width, h.height), s)
        pos = (pos + 3) // 4 * 4                          # word-storing routes: multiples of 4
        assert off == pos == int(r["out_off"]) and off % 4 == 0
        pos += w * hh * 3
        # the frame's own geometry stays
        assert (r["width"], r["height"], r["mcus_x"], r["mcus_y"]) == (h.width, h.height, h.mcus_x, h.mcus_y)
        assert list(r["h"][:h.ncomp]) == [a for a, _ in h.comp_hv] and list(r["v"][:h.ncomp]) == [b for _, b in h.comp_hv]
        # planes at the per-component n, each a multiple of 16 bytes
        want = [-(-(h.mcus_x * n * a) * (h.mcus_y * n * b) // 16) * 16
                for (a, b), (n, _, _) in zip(h.comp_hv, J.scaled_components(h.comp_hv, s))]
        assert J.scaled_plane_bytes(h, s) == want
        assert int(r["plane_off"]) == planes and planes % 16 == 0
        planes += sum(want)
        if s > 1:
            assert sum(want) < sum(J.scaled_plane_bytes(h, 1))
        assert sum(J.scaled_plane_bytes(h, 1)) == 64 * h.mcus_x * h.mcus_y * sum(a * b for a, b in h.comp_hv)
    assert out_bytes == pos and tot["total_plane_bytes"] == planes
    sizes = [J.scaled_size((h.width, h.height), s) for h, s in zip(hdrs, scales)]
    assert (tot["max_width"], tot["max_height"]) == (max(w for w, _ in sizes), max(h for _, h in sizes))


def _ranges(hdrs, blobs):
    offs, ends, pos = [], [], 0
    for h, b in zip(hdrs, blobs):
        offs.append(pos + h.data_offset)
        pos += len(b)
        ends.append(pos)
    return offs, ends


@pytest.mark.parametrize("kind", ["layout", "cmyk"])
def test_baseline_packers_place_a_mixed_scale_batch(kind):
    names, dtype = (PACK if kind == "layout" else PACK4), J.HEADER_ANY_DTYPE
    cases = [M.CASES[n] for n, _ in names]
    scales = [s for _, s in names]
    blobs = [c.baseline() for c in cases]
    hdrs = [J.parse(b, **c.kw) for b, c in zip(blobs, cases)]
    assert all(h.kind == J.DEVICE for h in hdrs)
    offs, ends = _ranges(hdrs, blobs)
    rec, tot, out_offs, out_bytes = J.pack_headers(hdrs, offs, ends, 2048, scales, dtype=dtype)
    _check_records(rec, tot, out_offs, out_bytes, hdrs, scales)
    full = J.pack_headers(hdrs, offs, ends, 2048, dtype=dtype)
    ones = J.pack_headers(hdrs, offs, ends, 2048, [1] * len(hdrs), dtype=dtype)
    assert ones[0].tobytes() == full[0].tobytes() and ones[1:] == full[1:]
    for k in ("total_blocks", "max_blocks", "total_units", "total_scan_bytes"):       # the entropy stages do not change
        assert tot[k] == full[1][k]
    with pytest.raises(ValueError):
        J.pack_headers(hdrs, offs, ends, 2048, [3] + scales[1:], dtype=dtype)


def test_progressive_any_packer_places_a_mixed_scale_batch():
    names = PACK[:3] + PACK4[:3]
    cases = [M.CASES[n] for n, _ in names]
    scales = [s for _, s in names]
    hdrs = [J.parse_progressive(c.progressive(), **c.kw) for c in cases]
    assert all(h.kind == J.DEVICE for h in hdrs)
    rec, srec, trec, tot, out_offs, out_bytes = J.pack_progressive(hdrs, [0] * len(hdrs), scales,
                                                                   dtype=J.PROG_HEADER_ANY_DTYPE)
    _check_records(rec, tot, out_offs, out_bytes, hdrs, scales)
    full = J.pack_progressive(hdrs, [0] * len(hdrs), dtype=J.PROG_HEADER_ANY_DTYPE)
    assert full[1].tobytes() == srec.tobytes() and full[2].tobytes() == trec.tobytes()
    assert tot["total_blocks"] == full[3]["total_blocks"]


def test_plan_carries_the_scales_of_every_group():
    c3, c4 = M.CASES["440-93x67"], M.CASES["photoshop-ycck-93x67"]
    groups = [[c4.baseline()], [c3.baseline()], [c3.progressive(), c4.progressive()]]
    kws = [[c4.kw], [c3.kw], [c3.kw, c4.kw]]
    ch, lh = ([J.parse(b, **k) for b, k in zip(g, kw)] for g, kw in zip(groups[:2], kws[:2]))
    ah = [J.parse_progressive(b, **k) for b, k in zip(groups[2], kws[2])]
    scales = [2, 4, 8, 1]
    own_pany = [("own", ch + lh, groups[0] + groups[1]), ("pany", ah, groups[2])]
    p = J.plan_device_batch(own_pany, 2048, scales)
    own, pany = p.group("own"), p.group("pany")
    assert p.scale_off is not None and p.scale_off % 256 == 0
    sec = dict(p.sections)
    assert list(sec[p.scale_off]) == [1, 2, 3, 0]
    spans = sorted((o, o + a.nbytes) for o, a in p.sections) + [(p.data_off, p.total)]
    assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(spans, spans[1:]))
    every = ch + lh + ah
    sizes = [J.scaled_size((h.width, h.height), s) for h, s in zip(every, scales)]
    assert all(o % 4 == 0 for o in p.out_offs)
    for (w, h), a, b in zip(sizes, p.out_offs, p.out_offs[1:] + [pany.out_off + pany.out_bytes]):
        assert a + w * h * 3 <= b
    first, second = (w * h * 3 for w, h in sizes[:2])      # one group now: the second image on the next whole word
    assert own.out_bytes == (first + 3) // 4 * 4 + second and p.out_offs[:2] == [own.out_off, own.out_off + (first + 3) // 4 * 4]
    assert (own.tot["max_width"], own.tot["max_height"]) == tuple(max(a, b) for a, b in zip(sizes[0], sizes[1]))
    assert pany.out_off == J.pad256(own.out_off + own.out_bytes) and (own.first, pany.first) == (0, 2)
    # full size: the plan of the call without scales, with no scale section
    q = J.plan_device_batch(own_pany, 2048, [])
    one = J.plan_device_batch(own_pany, 2048, [1] * 4)
    assert q.scale_off is None and one.scale_off is None and q.total == one.total and q.out_offs == one.out_offs


# ------------------------------------------------------------------------------------------------------------
# the keyword
# ------------------------------------------------------------------------------------------------------------
def _mixed():
    c3, c4 = M.CASES["440-93x67"], M.CASES["photoshop-ycck-93x67"]
    common = H.encode(H.smooth_rgb(67, 93, seed=1), quality=90, subsampling=2)
    return [common, c3.baseline(), c4.baseline(), c3.progressive(), c4.progressive()]


ALL_ON = dict(progressive="device", non_rgb="convert", cmyk="device", layouts="all")
OWN_ROUTES = ["device-layout", "device-cmyk", "device-progressive-layout", "device-progressive-cmyk"]


def test_a_bad_draft_layouts_value_raises():
    with pytest.raises(ValueError, match="draft_layouts must be 'common' or 'all', not 'some'"):
        J.check_draft_layouts("some")
    with pytest.raises(ValueError, match="draft_layouts must be"):
        J.plan_routes(_mixed(), draft=(23, 16), draft_layouts="every", **ALL_ON)
    with pytest.raises(ValueError, match="draft_layouts must be"):
        J.plan_routes(_mixed(), draft_layouts=None, **ALL_ON)
    assert J.check_draft_layouts("common") == "common" and J.check_draft_layouts("all") == "all"


def test_common_plans_these_files_as_host_under_a_draft():
    for kw in ({}, {"draft_layouts": "common"}):
        rp = J.plan_routes(_mixed(), draft=(23, 16), **ALL_ON, **kw)
        assert rp.routes == ["device"] + ["host"] * 4
        assert rp.scales == [4, 1, 1, 1, 1] and rp.order == [0]
        assert all(h.kind == J.HOST for h in rp.hdrs[1:])


def test_all_without_a_draft_changes_nothing():
    a = J.plan_routes(_mixed(), **ALL_ON)
    b = J.plan_routes(_mixed(), draft_layouts="all", **ALL_ON)
    assert a.routes == b.routes == ["device"] + OWN_ROUTES and a.scales == b.scales == [1] * 5
    assert [(type(h), h.kind, h.comp_hv, h.layout, h.ycck) for h in a.hdrs] == \
        [(type(h), h.kind, h.comp_hv, h.layout, h.ycck) for h in b.hdrs]
    # ... and nothing for a caller who did not opt in to the kinds themselves
    c = J.plan_routes(_mixed(), draft=(23, 16), draft_layouts="all", progressive="device")
    assert c.routes == ["device", "host", "black", "host", "black"]


def test_all_plans_them_as_their_device_routes_at_the_draft_scale():
    """Fails without the feature: under a draft these files are host kinds."""
    blobs = _mixed()
    for req, s in (((46, 33), 2), ((23, 16), 4), ((11, 8), 8), ((93, 67), 1)):
        rp = J.plan_routes(blobs, draft=req, draft_layouts="all", **ALL_ON)
        assert rp.routes == ["device"] + OWN_ROUTES
        assert rp.scales == [J.draft_scale((93, 67), req)] * 5 == [s] * 5
        assert rp.sizes == [J.scaled_size((93, 67), s)] * 5
        assert (rp.base, rp.own, rp.pany, rp.prog) == ([0], [1, 2], [3, 4], [])
        assert [rp.hdrs[i].ncomp for i in rp.own] == [3, 4]              # the layout and the cmyk file, in input order
        order = rp.order
        plan = J.plan_device_batch([(kind, [rp.hdrs[i] for i in idx], [blobs[i] for i in idx]) for kind, idx in rp.groups],
                                   2048, [rp.scales[i] for i in order])
        w, h = rp.sizes[0]
        two = (w * h * 3 + 3) // 4 * 4 + w * h * 3
        assert (plan.group("own").out_bytes, plan.group("pany").out_bytes) == (two, two)
        if s > 1:
            assert list(dict(plan.sections)[plan.scale_off]) == [s.bit_length() - 1] * 5
        else:
            assert plan.scale_off is None
    # an oversized drafted image goes to PIL, by the drafted size
    rp = J.plan_routes(blobs, draft=(23, 16), draft_layouts="all", max_bytes=24 * 17 * 3 - 1, **ALL_ON)
    assert rp.routes == ["host"] * 5
    rp = J.plan_routes(blobs, draft=(23, 16), draft_layouts="all", max_bytes=24 * 17 * 3, **ALL_ON)
    assert rp.routes == ["device"] + OWN_ROUTES


# ------------------------------------------------------------------------------------------------------------
# C entry points
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_scaled_entry_points_are_exported_and_reject_null_arguments(lib):
    from on_device_image_captioning_amd import _hip
    header = open(os.path.join(H.ROOT, "include", "odic_hip.h")).read()
    names = ("odic_jpeg_any_decode_scaled", "odic_jpeg_decode_progressive_any_scaled")
    for name in names:
        assert name in _hip.EXPORTED_SYMBOLS and len(getattr(lib, name).argtypes) == 5
        assert f"int {name}(" in header and header.index(name) < header.index("#define ODIC_ABI_VERSION")   # history line
        assert getattr(lib, name)(None, None, None, 0, None) == -2
    b = _hip.JpegBatch()
    b.headers, b.data, b.out, b.status = 16, 16, 16, 16
    b.n_images, b.subseq_bits, b.max_sync_passes = 1, 512, 4
    b.max_units = b.max_intervals = b.max_width = b.max_height = 1
    b.max_blocks = b.max_scan_bytes = b.total_scan_bytes = b.total_intervals = b.total_units = 1
    b.total_blocks = b.total_plane_bytes = 1
    for name, query in (("odic_jpeg_any_decode_scaled", lib.odic_jpeg_any_workspace_bytes),):
        fn, need = getattr(lib, name), query(ctypes.byref(b))
        assert need > 0
        assert fn(ctypes.byref(b), None, 16, need, None) == -2         # null scale_log2
        assert fn(ctypes.byref(b), 16, None, need, None) == -2         # no workspace
        assert fn(ctypes.byref(b), 16, 16, need - 1, None) == -1       # workspace too small
    p = _hip.JpegProgBatch()
    fn = lib.odic_jpeg_decode_progressive_any_scaled
    assert fn(ctypes.byref(p), 16, 16, 1 << 20, None) == -2            # null records
    p.headers = p.scans = p.tables = p.data = p.out = p.status = 16
    assert fn(ctypes.byref(p), None, 16, 1 << 20, None) == -2          # null scale_log2
    assert fn(ctypes.byref(p), 16, 16, 1 << 20, None) == -1            # empty descriptor
