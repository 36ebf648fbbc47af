"""CPU checks of the progressive JPEG writer (jpeg_writer.write_progressive_jpeg) and of the corpus it writes
(tests/jpeg_prog_stream_cases.py): Pillow opens every file, `jpeg.parse_progressive` sorts it as the expected route
implies and finds the scans and dependency levels the case states, the model of test_jpeg_progressive_host.py reads back
the very coefficients the writer was given and turns them into Pillow's pixels, the mask formulation of AC refinement
(what prog_ac_refine does) equals the walk on every refinement scan, and the writer's records describe the bytes.
Writer, model and Pillow are checked against each other here before test_jpeg_prog_streams_gpu.py brings the device in."""
import io
import warnings

import numpy as np
import pytest
from PIL import Image

import jpeg_prog_stream_cases as C
import jpeg_writer as W
import test_jpeg_host as H
import test_jpeg_progressive_host as P
from on_device_image_captioning_amd import jpeg as J

N_HOST = 7                                                 # "host" by design: jpeg_prog_stream_cases.py lists them
PARSER_REASONS = {"host_no_ac_scans": "incomplete scan script", "host_missing_last_refinement": "incomplete scan script",
                  "host_65_scans": "more than 64 scans", "host_ac_before_dc": "AC scan before DC",
                  "host_ah_mismatch": "bogus progression: Ah does not continue the previous scan"}
# what the model trips over in the two files the device turns away itself
MODEL_FAILURES = {"host_refine_size2": "assert s == 1", "host_run_past_se": "assert kk <= sc.se"}


def pil_rgb(blob):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        im = Image.open(io.BytesIO(blob))
        assert im.mode == "RGB"
        return np.asarray(im)


def model_rgb(blob, hd, coef):
    """The model's pixels for progressive coefficients: the baseline model's DC prediction, IDCT, planes and colour
    stages, as test_jpeg_progressive_host.model_of runs them (raises H.Rejected outside the device's IDCT range)."""
    base, diffs = P.as_baseline(hd, coef)
    assert np.array_equal(H.model_dc_prediction(diffs, base), coef)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(J, "parse", lambda b: base)
        mp.setattr(H, "model_coefficients", lambda b, h: diffs)
        return H.model_rgb(blob)
    finally:
        mp.undo()


def test_the_corpus_covers_what_it_names():
    names = list(C.CASES)
    assert len(names) == len(set(names)) >= 70
    hosts = C.names(C.HOST)
    assert len(hosts) == N_HOST and set(hosts) == set(PARSER_REASONS) | set(MODEL_FAILURES)
    for n in hosts:
        rec = C.build(n)[2]
        assert rec["why_host"] and rec["host_by"] == ("parser" if n in PARSER_REASONS else "status")
    for prefix in ("std_", "dc_", "sa_", "eob_", "refine_", "bands_", "restart_", "huff_", "size_", "host_"):
        assert any(n.startswith(prefix) for n in names), prefix
    scans = [s for n in C.names(C.DEVICE) for s in C.build(n)[2]["scans"]]
    assert C.categories(scans) == set(range(15))                       # EOB0 .. EOB14
    assert max(n for s in scans for _, n in s["eob_runs"]) == 0x7FFF
    for kind in ("ac_first", "ac_refine"):
        assert C.categories(s for s in scans if s["kind"] == kind) >= {0, 1, 2, 3, 4, 14}, kind
    for kind in ("dc_first", "dc_refine", "ac_first", "ac_refine"):
        mine = [s for s in scans if s["kind"] == kind]
        assert any(s["n_intervals"] > 1 for s in mine) and any(s["n_intervals"] == 1 for s in mine), kind
        assert any(s["n_intervals"] == s["n_units"] > 1 for s in mine), kind              # an interval of one unit
    for kind in ("dc_first", "dc_refine"):
        for sampling in (0, 1, 2):
            masks = {sum(1 << c for c in s["comps"]) for n in C.names(C.DEVICE) if C.build(n)[2]["sampling"] == sampling
                     for s in C.build(n)[2]["scans"] if s["kind"] == kind}
            assert masks == set(range(1, 8)), (kind, sampling)
    refine = [s for s in scans if s["kind"] == "ac_refine"]
    assert {s["al"] for s in refine} >= {0, 1, 2} and max(s["max_correction_bits"] for s in refine) >= 63
    assert any(s["zrl"] for s in refine) and any(s["ss"] == s["se"] for s in refine)
    assert max(len(C.build(n)[2]["scans"]) for n in C.names(C.DEVICE)) == J.MAX_SCANS
    assert {16} in [set(ln) for s in scans for ln in s["lengths"].values() if ln]
    assert {k[1] for s in scans for k in s["tables"]} == {0, 1, 2, 3}
    for n in names:                                                    # small frames, but for the one that cannot be
        w, h = C.build(n)[2]["size"]
        assert (w <= 48 and h <= 40) or n in C.BIG, n


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_against_pillow_parser_and_model(name):
    """Building the case asserts its own precondition.  Then: Pillow yields an RGB image of the declared size; the
    parser gives the kind the route implies, with the stated reason for a host case of its own, else the stated number
    of scans and dependency levels; for a device case the model reads back the writer's input coefficients and its
    pixels are Pillow's."""
    blob, route, rec = C.build(name)
    want = pil_rgb(blob)
    w, h = rec["size"]
    assert want.shape == (h, w, 3)
    assert J.parse(blob).reason == "SOF2"
    hd = J.parse_progressive(blob)
    if route == C.HOST and rec["host_by"] == "parser":
        assert hd.kind == J.HOST and hd.reason == rec["reason"] == PARSER_REASONS[name]
        return
    assert hd.kind == J.DEVICE, hd.reason                  # a "status" host case is the device's to turn away
    assert (hd.width, hd.height, hd.sampling) == (w, h, rec["sampling"])
    assert len(hd.scans) == rec["n_scans"]
    if route == C.HOST:
        with pytest.raises(AssertionError) as e:
            P.model_progressive_coefficients(blob, hd)
        assert MODEL_FAILURES[name] in str(e.traceback[-1].statement)
        return
    assert hd.n_levels == rec["n_levels"]
    coef = P.model_progressive_coefficients(blob, hd)
    assert coef.shape == rec["coefs"].shape and np.array_equal(coef, rec["coefs"])
    got = model_rgb(blob, hd, coef)                        # raises Rejected outside the device's IDCT range
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want).max())


@pytest.mark.parametrize("name", [n for n in C.CASES if not n.startswith("host_")])
def test_mask_formulation_of_ac_refinement_equals_the_walk_on_the_corpus(name):
    """Every AC refinement scan of the case, decoded with the device's formulation (test_jpeg_progressive_host.
    refine_block_with_masks) on top of the walk's coefficients for the scans before it: the walk's coefficients."""
    blob, route, rec = C.build(name)
    hd = J.parse_progressive(blob)
    nat = J.NATURAL_ORDER
    prefix = J.ProgHeader(J.DEVICE, width=hd.width, height=hd.height, ncomp=3, sampling=hd.sampling, comp_ids=hd.comp_ids,
                          comp_hv=hd.comp_hv, qtables=hd.qtables)
    for n, sc in enumerate(hd.scans):
        if not (sc.ss and sc.ah):
            continue
        prefix.scans = hd.scans[:n]
        coef = P.model_progressive_coefficients(blob, prefix)
        segs, _ = P.walk_entropy(blob, sc.data_offset)
        R = sc.restart_interval or sc.n_units
        tab = J.device_tables(sc.ac_table)
        for i, seg in enumerate(segs):
            br, eobrun = P.BitReader(seg), 0
            for u in range(i * R, min((i + 1) * R, sc.n_units)):
                b = P.block_index(hd, sc.comps[0], u, sc.blocks_w)
                zz = [int(x) for x in coef[b, nat]]
                eobrun = P.refine_block_with_masks(zz, br, tab, sc.ss, sc.se, sc.al, eobrun)
                coef[b, nat] = zz
            assert br.pos <= br.n
        prefix.scans = hd.scans[:n + 1]
        assert np.array_equal(coef, P.model_progressive_coefficients(blob, prefix)), n
    assert any(s["kind"] == "ac_refine" for s in rec["scans"]) == any(sc.ss and sc.ah for sc in hd.scans)


@pytest.mark.parametrize("name", list(C.CASES))
def test_the_records_describe_the_bytes(name):
    """An independent marker walk (test_jpeg_progressive_host.walk) finds every scan where the record says it is, with
    the header, the tables, the restart interval and the intervals it states; the 0xFF bytes of the data are the
    stuffed pairs and RST markers it lists."""
    blob, _, rec = C.build(name)
    scans, eoi = P.walk(blob)
    assert len(scans) == len(rec["scans"]) and blob[eoi:] == b"\xff\xd9"
    for wk, r in zip(scans, rec["scans"]):
        assert wk["sos"] == r["sos_offset"] and wk["start"] == r["data_offset"]
        assert wk["end"] == r["data_offset"] + r["scan_len"]
        assert tuple(i - 1 for i in wk["ids"]) == r["comps"]                  # JFIF ids 1, 2, 3
        assert (wk["ss"], wk["se"], wk["ah"], wk["al"], wk["dri"]) == (r["ss"], r["se"], r["ah"], r["al"], r["restart"])
        assert len(wk["segs"]) == r["n_intervals"] == len(r["rst"]) + 1 == len(r["interval_bytes"])
        assert r["kind"] == ("dc_" if r["ss"] == 0 else "ac_") + ("refine" if r["ah"] else "first")
        for (tc, ti), table in r["tables"].items():
            assert wk["dht"][(tc, ti)] == table
            assert (tc, ti) in [(0, td) for td, _ in wk["tsel"]] + [(1, wk["tsel"][0][1])]
        assert set(r["defined"]) <= set(r["tables"])
        body = np.frombuffer(blob[r["data_offset"]:r["data_offset"] + r["scan_len"] + 1], np.uint8)
        ff = np.flatnonzero(body[:-1] == 0xFF)
        assert sorted(r["ff00"] + r["rst"]) == ff.tolist()
        assert all(body[i + 1] == 0 for i in r["ff00"])
        assert [int(body[i + 1]) for i in r["rst"]] == [0xD0 + k % 8 for k in range(len(r["rst"]))]
        assert sum(r["interval_bytes"]) + 2 * len(r["rst"]) == r["scan_len"]
        emitted = sum(sum(v.values()) for v in r["lengths"].values())
        assert emitted == sum(sum(v.values()) for v in r["symbols"].values())
        assert (emitted > 0) == (r["kind"] != "dc_refine")
        eobs = sum(n for k, v in r["symbols"].items() if k[0] == 1 for s, n in v.items() if s & 15 == 0 and s >> 4 < 15)
        assert eobs == len(r["eob_runs"]) and all((1 << c) <= n < (2 << c) for c, n in r["eob_runs"])
        assert r["zrl"] == sum(v[W.ZRL] for k, v in r["symbols"].items() if k[0] == 1)


def dc_values(coefs, sampling):
    """The DC differences `coefficients_from_pixels` returns (no restart interval) → blocks with the DC value."""
    out = []
    for blocks in coefs:
        b = np.array(blocks, np.int64)
        b[:, 0] = np.cumsum(b[:, 0])
        out.append(b)
    return out


@pytest.mark.parametrize("sampling", [0, 1, 2], ids=C.SAMPLING_NAMES)
@pytest.mark.parametrize("restart", [0, 3])
def test_standard_script_files_parse_like_a_pillow_save(sampling, restart):
    """libjpeg's ten-scan script through this writer and the same picture through Pillow's progressive save with the
    same quantisation tables, sampling and restart interval: the same frame, and scan by scan the same components,
    band, Ah / Al, restart interval, units, raster width and dependency level; the writer's coefficients come back."""
    size = (43, 29)
    img = H.smooth_rgb(size[1], size[0], seed=1)
    qt = [np.full(64, 3, np.int64), np.full(64, 5, np.int64), np.full(64, 5, np.int64)]
    ref = J.parse_progressive(P.encode_progressive(img, qtables=[[int(v) for v in q] for q in qt[:2]],
                                                   subsampling=sampling, restart_marker_blocks=restart))
    coefs = dc_values(W.coefficients_from_pixels(img, sampling, qt), sampling)
    blob, recs = W.write_progressive_jpeg(*size, sampling, coefs, qt, W.standard_script(restart))
    mine = J.parse_progressive(blob)
    assert ref.kind == mine.kind == J.DEVICE, (ref.reason, mine.reason)
    for f in ("width", "height", "sampling", "comp_ids", "comp_hv", "n_levels"):
        assert getattr(ref, f) == getattr(mine, f), f
    assert all(list(a) == list(b) for a, b in zip(ref.qtables, mine.qtables))
    assert len(ref.scans) == len(mine.scans) == 10
    for a, b in zip(ref.scans, mine.scans):
        for f in ("comps", "ss", "se", "ah", "al", "restart_interval", "level", "n_units", "blocks_w", "n_intervals"):
            assert getattr(a, f) == getattr(b, f), f
        assert [t is None for t in a.dc_tables] == [t is None for t in b.dc_tables]
        assert (a.ac_table is None) == (b.ac_table is None)
    assert np.array_equal(P.model_progressive_coefficients(blob, mine), W.interleave_values(coefs, sampling))
    got = model_rgb(blob, mine, P.model_progressive_coefficients(blob, mine))
    assert np.array_equal(got, pil_rgb(blob))


def test_writer_refuses_symbol_lists_that_do_not_code_the_coefficients():
    size = (16, 8)
    coefs = C.blank(size, 0)
    coefs[0][0, 2] = 3
    S = W.Scan
    dc = S((0, 1, 2), 0, 0, 0, 0)
    rest = [S((1,), 1, 63, 0, 0), S((2,), 1, 63, 0, 0)]
    ok = [dc, S((0,), 1, 63, 0, 0, symbols={0: [(0x12, 3)]})] + rest
    blob, recs = W.write_progressive_jpeg(*size, 0, coefs, C.ONES, ok)
    assert recs[1]["symbols"][(1, 0)] == {0x12: 1, 0x10: 1} and recs[1]["eob_runs"] == [(1, 2)]
    hd = J.parse_progressive(blob)
    assert np.array_equal(P.model_progressive_coefficients(blob, hd), W.interleave_values(coefs, 0))
    for bad in ({0: [(0x02, 3)]}, {0: [(0x12, 2)]}, {0: [(0x10, 2)]}, {1: [(0x12, 3)]}):
        with pytest.raises(ValueError):
            W.write_progressive_jpeg(*size, 0, coefs, C.ONES, [dc, S((0,), 1, 63, 0, 0, symbols=bad)] + rest)
    with pytest.raises(ValueError, match="no EOB"):
        W.write_progressive_jpeg(*size, 0, coefs, C.ONES, [dc, S((0,), 1, 63, 0, 0, symbols={1: [(0x10, 5)]})] + rest)
    with pytest.raises(ValueError, match="one component"):
        W.write_progressive_jpeg(*size, 0, coefs, C.ONES, [dc, S((0, 1), 1, 63, 0, 0)])
