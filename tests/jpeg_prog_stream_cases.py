"""Progressive JPEG streams no Pillow save produces, written with jpeg_writer.write_progressive_jpeg: DC scans of one and
two components, successive approximation four stages deep, every EOBn category, EOB runs against restart intervals,
the corners of AC refinement, odd band splits, 64 scans, restart intervals in every scan kind, odd Huffman tables and
narrow frames under non-interleaved DC scans.  `build(name)` → (blob, expected route, record); every case asserts from
the writer's per-scan records (record["scans"]) that it still reaches what it was built for, and states how many scans
and dependency levels the parser must find (record["n_scans"], record["n_levels"]: 1 for a first DC scan, one more for
every scan that has to wait for another of its component and band, so 1 + the longest such chain).

Expected route: "device" for every legal, complete script.  "host" by design, with the reason in record["why_host"]
and who hands the file over in record["host_by"] ("parser": jpeg.parse_progressive gives record["reason"]; "status":
the device sets its status word and Pillow decodes the file again):

    host_refine_size2            an AC refinement symbol of size 2: libjpeg warns and reads on, prog_ac_refine refuses
    host_run_past_se             a run/size that lands behind Se: libjpeg writes outside the band, prog_ac_first refuses
    host_no_ac_scans             DC scans only: libjpeg smooths across blocks
    host_missing_last_refinement the standard script without its last scan: the same
    host_65_scans                one scan more than MAX_SCANS
    host_ac_before_dc            libjpeg warns about the progression
    host_ah_mismatch             a refinement whose Ah is not the Al before it: the same

All quantisation entries are 1 and the coefficients small, so every device case stays far inside kIdctLimit.
"""
import functools

import numpy as np

import jpeg_writer as W
from jpeg_stream_cases import DEVICE, HOST, ONES, SAMPLING_NAMES
from jpeg_writer import Scan

CASES = {}
BIG = ("eob_big_444",)                                     # the one frame large enough for EOB14 and a run of 32767


def case(name):
    def deco(fn):
        assert name not in CASES
        CASES[name] = fn
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def build(name):
    blob, route, rec = CASES[name]()
    assert route in (DEVICE, HOST)
    assert (route == HOST) == ("why_host" in rec), name
    assert len(rec["scans"]) == rec["n_scans"], (name, len(rec["scans"]))
    return blob, route, rec


def names(route=None):
    return [n for n in CASES if route is None or build(n)[1] == route]


# ------------------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------------------
def n_mcus(size, sampling):
    hy, vy = W.LUMA_HV[sampling]
    return -(-size[0] // (8 * hy)) * -(-size[1] // (8 * vy))


def blank(size, sampling):
    n = n_mcus(size, sampling)
    return [np.zeros((n * W.LUMA_BLOCKS[sampling], 64), np.int64), np.zeros((n, 64), np.int64),
            np.zeros((n, 64), np.int64)]


def noise(size, sampling, seed, amp=6, density=0.35, dc=30):
    """Sparse noise: AC values in ±amp with the given density, DC values in ±dc.  Blocks outside a component's own raster
    (the padding of the last MCU column and row) stay zero: non-interleaved scans never send them."""
    rng = np.random.default_rng(seed)
    coefs = blank(size, sampling)
    for c, blocks in enumerate(coefs):
        own = W.raster_to_mcu_order(*size, sampling, c)
        v = rng.integers(-amp, amp + 1, (len(own), 64)) * (rng.random((len(own), 64)) < density)
        v[:, 0] = rng.integers(-dc, dc + 1, len(own))
        blocks[own] = v
    return coefs


def finish(blob, recs, size, sampling, coefs, n_scans, n_levels, **more):
    rec = dict(scans=recs, size=size, sampling=sampling, n_scans=n_scans, n_levels=n_levels, **more)
    rec["coefs"] = W.interleave_values(coefs, sampling) if coefs is not None else None
    return blob, rec


def device(size, sampling, coefs, script, n_scans, n_levels, **kw):
    blob, recs = W.write_progressive_jpeg(*size, sampling, coefs, ONES, script, **kw)
    blob, rec = finish(blob, recs, size, sampling, coefs, n_scans, n_levels)
    return blob, DEVICE, rec


def host(size, sampling, coefs, script, n_scans, by, why, reason=None):
    blob, recs = W.write_progressive_jpeg(*size, sampling, coefs, ONES, script)
    blob, rec = finish(blob, recs, size, sampling, None, n_scans, 0, host_by=by, why_host=why, reason=reason)
    return blob, HOST, rec


def simple_script(groups, al_dc=0, restart=0):
    """One first DC scan per group of components at Al = al_dc, a full AC scan per component, then the DC refinements
    group by group down to Al = 0."""
    s = [Scan(g, 0, 0, 0, al_dc, restart) for g in groups]
    s += [Scan((c,), 1, 63, 0, 0, restart) for c in range(3)]
    for al in range(al_dc - 1, -1, -1):
        s += [Scan(g, 0, 0, al + 1, al, restart) for g in groups]
    return s


def kinds(rec, kind):
    return [s for s in rec["scans"] if s["kind"] == kind]


def categories(scans):
    return {r for s in scans for r, _ in s["eob_runs"]}


# ------------------------------------------------------------------------------------------------------------
# the standard script through this writer
# ------------------------------------------------------------------------------------------------------------
def _std_case(sampling):
    def fn():
        size = (40, 24)
        return device(size, sampling, noise(size, sampling, seed=sampling), W.standard_script(), 10, 4)
    return fn


for _s in (0, 1, 2):
    case(f"std_{SAMPLING_NAMES[_s]}")(_std_case(_s))


# ------------------------------------------------------------------------------------------------------------
# DC scans of one, two and three components: every component mask, first pass and refinement
# ------------------------------------------------------------------------------------------------------------
def _dc_mask_case(mask, sampling):
    def fn():
        size = (35, 21)                                    # 4:2:0: luma raster 5 x 3 blocks inside 6 x 4 of the MCUs
        inside = tuple(c for c in range(3) if (mask >> c) & 1)
        rest = tuple(c for c in range(3) if not (mask >> c) & 1)
        groups = [inside] + ([rest] if rest else [])
        blob, route, rec = device(size, sampling, noise(size, sampling, seed=mask), simple_script(groups, al_dc=1),
                                  2 * len(groups) + 3, 2)
        for kind in ("dc_first", "dc_refine"):
            assert inside in [s["comps"] for s in kinds(rec, kind)]
        first = kinds(rec, "dc_first")[0]
        assert first["comps"] == inside and len(first["tables"]) == len({(0, 1, 1)[c] for c in inside})
        if len(inside) == 1 and sampling:                  # the component's own raster is not the MCU-padded array
            assert first["n_units"] == len(W.raster_to_mcu_order(*size, sampling, inside[0]))
            assert inside[0] != 0 or first["n_units"] < n_mcus(size, sampling) * W.LUMA_BLOCKS[sampling]
        return blob, route, rec
    return fn


for _mask in range(1, 8):
    for _s in (0, 1, 2):
        case(f"dc_mask{_mask}_{SAMPLING_NAMES[_s]}")(_dc_mask_case(_mask, _s))


# ------------------------------------------------------------------------------------------------------------
# successive approximation four stages deep
# ------------------------------------------------------------------------------------------------------------
def _sa_case(sampling):
    def fn():
        size = (35, 21)
        coefs = noise(size, sampling, seed=10 + sampling, amp=15, density=0.4, dc=100)
        own = W.raster_to_mcu_order(*size, sampling, 0)
        coefs[0][own[0], 5], coefs[0][own[1], 7], coefs[0][own[1], 0] = -11, -15, -93
        S = Scan
        script = [S((0, 1, 2), 0, 0, 0, 3), S((0,), 1, 63, 0, 3), S((1,), 1, 63, 0, 2), S((2,), 1, 63, 0, 2)]
        for al in (2, 1, 0):
            script += [S((0, 1, 2), 0, 0, al + 1, al), S((0,), 1, 63, al + 1, al)]
            if al < 2:
                script += [S((1,), 1, 63, al + 1, al), S((2,), 1, 63, al + 1, al)]
        blob, route, rec = device(size, sampling, coefs, script, 14, 5)
        assert {s["al"] for s in kinds(rec, "ac_refine")} == {0, 1, 2} == {s["al"] for s in kinds(rec, "dc_refine")}
        y = coefs[0][own, 1:]
        twice = (y < 0) & (np.abs(y) >> 3 > 0) & ((np.abs(y) & 1) + ((np.abs(y) >> 1) & 1) + ((np.abs(y) >> 2) & 1) >= 2)
        assert twice.any()                                 # a negative value corrected at two stages or more
        return blob, route, rec
    return fn


for _s in (0, 1, 2):
    case(f"sa_deep_{SAMPLING_NAMES[_s]}")(_sa_case(_s))


# ------------------------------------------------------------------------------------------------------------
# EOB runs
# ------------------------------------------------------------------------------------------------------------
@case("eob_small_444")
def _eob_small():
    """EOB0 .. EOB4 with their appended bits on 30 blocks a component: runs cut short in the first pass (Y, Cb) and in
    refinement (Cr), where blocks that hold nothing but correction bits lie inside the runs."""
    size = (48, 40)
    coefs = noise(size, 0, seed=20, density=0.0, dc=12)
    coefs[0][0, 3], coefs[1][0, 1] = 5, -2
    coefs[2][0, 2] = 3
    for b in (3, 4, 8, 17, 25):                            # nonzero before the refinement, no new coefficient in it
        coefs[2][b, 1 + b % 7], coefs[2][b, 30 + b] = 2, -3
    script = [Scan((0, 1, 2), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 0, cut=(1, 2, 5, 10)),
              Scan((1,), 1, 63, 0, 0, cut=(13,)), Scan((2,), 1, 63, 0, 1), Scan((2,), 1, 63, 1, 0, cut=(1, 2, 5, 10))]
    blob, route, rec = device(size, 0, coefs, script, 5, 3)
    y, cb, cr = rec["scans"][1], rec["scans"][2], rec["scans"][4]
    # a run counts the block whose EOB opens it: block 0's rest is a run of its own in front of the first cut
    assert y["eob_runs"] == [(0, 1), (0, 1), (1, 3), (2, 5), (4, 20)] and cb["eob_runs"] == [(3, 13), (4, 17)]
    assert cr["kind"] == "ac_refine" and cr["eob_runs"] == y["eob_runs"]
    assert cr["max_correction_bits"] >= 4                  # blocks 3 and 4 share a run: their bits follow one symbol
    return blob, route, rec


@case("eob_big_444")
def _eob_big():
    """EOB5 .. EOB14 and a run of 32767 need 32768 blocks of one component: 1024 x 2048, all AC zero outside a few
    blocks.  Y: runs of 32, 64 .. 8192 cut short, then 16415 (EOB14).  Cb: no AC at all, so the encoder's run reaches
    0x7FFF, is flushed, and one block is left.  Cr: runs of thousands of blocks in a refinement scan."""
    size = (1024, 2048)
    coefs = blank(size, 0)
    rng = np.random.default_rng(21)
    for c in range(3):
        coefs[c][:, 0] = rng.integers(-3, 4, len(coefs[c])) * (rng.random(len(coefs[c])) < 0.01)
    coefs[0][0, 1] = 4
    cuts, at = [1], 1
    for r in range(5, 14):
        at += 1 << r
        cuts.append(at)
    coefs[2][100, 1], coefs[2][100, 2], coefs[2][20000, 9], coefs[2][20000, 10] = 2, 1, -3, -1
    script = [Scan((0, 1, 2), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 0, cut=tuple(cuts)), Scan((1,), 1, 63, 0, 0),
              Scan((2,), 1, 63, 0, 1), Scan((2,), 1, 63, 1, 0)]
    blob, route, rec = device(size, 0, coefs, script, 5, 3)
    y, cb, cr = rec["scans"][1], rec["scans"][2], rec["scans"][4]
    assert y["eob_runs"] == [(0, 1)] + [(r, 1 << r) for r in range(5, 14)] + [(14, 16415)]
    assert cb["eob_runs"] == [(14, 32767), (0, 1)]
    assert cr["eob_runs"] == [(6, 100), (14, 19900), (13, 12768)]     # a run counts the block whose EOB opens it
    return blob, route, rec


@case("eob_intervals_444")
def _eob_intervals():
    """30 blocks in restart intervals of 10.  First pass (Y) and refinement (Cb): a run that ends exactly at an
    interval's last block, a run that starts afresh at an interval's first block, and an EOB3 that announces 12 blocks
    where 4 remain in the interval."""
    size = (48, 40)
    coefs = noise(size, 0, seed=22, density=0.0, dc=12)
    for c, one in ((0, 1), (1, 2)):
        coefs[c][3, 4], coefs[c][15, 2] = 3 * one, -2 * one
    coefs[1][5, 7], coefs[1][12, 3], coefs[1][18, 9], coefs[1][25, 1] = 2, -3, 2, 3          # corrections inside the runs
    coefs[1][15, 6] = 1                                                                    # new in the refinement
    coefs[2][7, 1] = 2
    announce = {16: [(0x30, 12)]}
    script = [Scan((0, 1, 2), 0, 0, 0, 0, 4), Scan((0,), 1, 63, 0, 0, 10, symbols=announce),
              Scan((1,), 1, 63, 0, 1, 10), Scan((1,), 1, 63, 1, 0, 10, symbols=announce),
              Scan((2,), 1, 63, 0, 0, 10)]
    blob, route, rec = device(size, 0, coefs, script, 5, 3)
    # Y: blocks 0-2 | 3's rest and 4-9, to the interval's end || 10-14 from its start | 15's rest | 16-19 announced
    # as 12 || 20-29.  Cb's refinement: 0-9 are one run of correction bits
    assert rec["scans"][1]["eob_runs"] == [(1, 3), (2, 7), (2, 5), (0, 1), (3, 12), (3, 10)]
    assert rec["scans"][3]["eob_runs"] == [(3, 10), (2, 5), (0, 1), (3, 12), (3, 10)]
    assert all(rec["scans"][k]["n_intervals"] == 3 for k in (1, 2, 3, 4))
    assert rec["scans"][3]["kind"] == "ac_refine" and rec["scans"][3]["max_correction_bits"] >= 1
    return blob, route, rec


# ------------------------------------------------------------------------------------------------------------
# AC refinement corners
# ------------------------------------------------------------------------------------------------------------
@case("refine_corners_444")
def _refine_corners():
    size = (40, 32)
    coefs = noise(size, 0, seed=23, density=0.0, dc=12)
    y, cb = coefs[0], coefs[1]
    old = np.where(np.arange(63) % 2, 2, -3)               # nonzero before the refinement: one correction bit each
    zeros10 = [2, 9, 17, 18, 30, 41, 42, 55, 60, 63]
    y[0, 1:] = old                                         # block 0: ten zeros left, no new coefficient, a ZRL forced:
    y[0, zeros10] = 0                                      # it passes all ten and takes the 53 correction bits
    y[1, 1:21] = 0                                         # block 1: a new -1 at coefficient 63 behind 20 + 42 old ...
    y[1, 21:63], y[1, 63] = old[20:62], -1                 # ... a ZRL that is needed, then run 4
    y[2, 1:63], y[2, 63] = old[:62], 1                     # block 2: 62 old ones, a new one at 63: one symbol, 62 bits
    y[3, 1:] = old                                         # block 3: the whole band nonzero: an EOB, 63 bits behind it
    y[4, 2], y[4, 4], y[4, 10], y[4, 20] = 3, -1, -2, 2    # block 4: correction, new, EOB at k = 5, two corrections
    for b in (6, 7, 9):                                    # blocks 5 .. 9: a run; three hold correction bits only
        y[b, 5 + b], y[b, 40] = 2, -2
    cb[2, 3], cb[2, 20], cb[2, 21], cb[2, 63] = 2, -1, 1, 3          # new ones at the last / first coefficient of a band
    S = Scan
    script = [S((0, 1, 2), 0, 0, 0, 0), S((0,), 1, 63, 0, 1), S((0,), 1, 63, 1, 0, symbols={0: [(W.ZRL, None)]}, cut=(4, 10)),
              S((1,), 1, 20, 0, 1), S((1,), 21, 63, 0, 1), S((1,), 1, 20, 1, 0), S((1,), 21, 63, 1, 0), S((2,), 1, 63, 0, 0)]
    blob, route, rec = device(size, 0, coefs, script, 8, 3)
    r = rec["scans"][2]
    assert r["kind"] == "ac_refine" and r["zrl"] == 2 and r["max_correction_bits"] == 63
    assert r["symbols"][(1, 0)][0x41] == 1 and r["symbols"][(1, 0)][0x01] == 1 and r["symbols"][(1, 0)][0x21] == 1
    assert r["eob_runs"] == [(0, 1), (2, 6), (3, 10)]      # block 3 alone; the rest of 4 and 5 .. 9; 10 .. 19
    assert rec["scans"][5]["symbols"][(1, 1)][0x01 | (18 - 16) << 4] == 1 and rec["scans"][5]["zrl"] == 1
    assert rec["scans"][6]["symbols"][(1, 1)][0x01] == 1
    return blob, route, rec


# ------------------------------------------------------------------------------------------------------------
# bands
# ------------------------------------------------------------------------------------------------------------
def band_scans(c, edges, al=0):
    """First AC scans of component c over the bands [edges[i], edges[i + 1] - 1]."""
    return [Scan((c,), a, b - 1, 0, al) for a, b in zip(edges, edges[1:])]


@case("bands_single_coefficient_444")
def _bands_single():
    size = (40, 32)
    coefs = noise(size, 0, seed=24, amp=3, density=0.6)
    script = [Scan((0, 1, 2), 0, 0, 0, 0)] + band_scans(0, [1, 2]) + [Scan((0,), 2, 2, 0, 1)] + band_scans(0, [3, 4, 64])
    script += band_scans(1, [1, 6, 7, 64]) + band_scans(2, [1, 64]) + [Scan((0,), 2, 2, 1, 0)]
    blob, route, rec = device(size, 0, coefs, script, 10, 3)
    assert sum(s["ss"] == s["se"] for s in rec["scans"] if s["ss"]) == 5
    return blob, route, rec


def _bands_split_case(sampling):
    def fn():
        size = (35, 21)
        coefs = noise(size, sampling, seed=25 + sampling, amp=3, density=0.6)
        script = [Scan((0, 1, 2), 0, 0, 0, 0)] + band_scans(0, [1, 2, 3, 7, 16, 29, 41, 63, 64])
        script += band_scans(1, [1, 33, 64]) + band_scans(2, [1, 10, 11, 12, 60, 64])
        return device(size, sampling, coefs, script, 16, 2)
    return fn


for _s in (0, 1, 2):
    case(f"bands_split_{SAMPLING_NAMES[_s]}")(_bands_split_case(_s))


def many_scans(extra):
    """One DC scan and 21 bands of three coefficients for each component: 64 scans; `extra` splits Y's first band."""
    script = [Scan((0, 1, 2), 0, 0, 0, 0)]
    for c in range(3):
        script += band_scans(c, ([1, 2] if extra and c == 0 else [1]) + list(range(4, 65, 3)))
    return script


@case("bands_64_scans_444")
def _bands_64():
    size = (24, 16)
    return device(size, 0, noise(size, 0, seed=28, amp=3, density=0.6), many_scans(False), 64, 2)


# ------------------------------------------------------------------------------------------------------------
# restart intervals in every scan kind
# ------------------------------------------------------------------------------------------------------------
def _restart_case(sampling, intervals):
    def fn():
        size = (35, 21)
        script = W.standard_script()
        for sc, r in zip(script, intervals):
            sc.restart = r
        coefs = noise(size, sampling, seed=30 + sampling)
        blob, route, rec = device(size, sampling, coefs, script, 10, 4)
        assert {s["kind"] for s in rec["scans"] if s["n_intervals"] > 1} == {"dc_first", "dc_refine", "ac_first", "ac_refine"}
        for s in kinds(rec, "dc_refine"):                  # a few bits an interval, padded to a byte
            per = sum(W.LUMA_BLOCKS[sampling] if c == 0 else 1 for c in s["comps"])
            stuffed = sum(i < s["interval_bytes"][0] for i in s["ff00"])
            assert s["n_intervals"] > 1 and s["interval_bytes"][0] - stuffed == -(-per * s["restart"] // 8)
        changes = 1 + sum(a != b for a, b in zip(intervals, intervals[1:]))
        assert blob.count(b"\xff\xdd\x00\x04") == changes
        if len(set(intervals)) == 1:                       # an interval of one unit everywhere
            assert all(s["n_intervals"] == s["n_units"] for s in rec["scans"])
        return blob, route, rec
    return fn


for _s in (0, 1, 2):
    case(f"restart_one_unit_{SAMPLING_NAMES[_s]}")(_restart_case(_s, [1] * 10))
    case(f"restart_changes_{SAMPLING_NAMES[_s]}")(_restart_case(_s, [2, 3, 0, 1, 5, 4, 3, 7, 0, 2]))


# ------------------------------------------------------------------------------------------------------------
# Huffman tables
# ------------------------------------------------------------------------------------------------------------
@case("huff_redefined_same_id_h2v2")
def _huff_redefined():
    """Every AC scan names AC table 0 and every DC component DC table 0; each scan brings its own."""
    size = (35, 21)
    script = W.standard_script()
    for sc in script:
        sc.ids = (0,) * len(sc.comps) if sc.ss == 0 else 0
    blob, route, rec = device(size, 2, noise(size, 2, seed=40), script, 10, 4)
    ac = [s for s in rec["scans"] if s["ss"]]
    assert all(list(s["tables"]) == [(1, 0)] for s in ac)
    assert sum((1, 0) in s["defined"] for s in ac) >= 3 and len({s["tables"][(1, 0)][1] for s in ac}) >= 3
    return blob, route, rec


@case("huff_ids23_h2v1")
def _huff_ids23():
    size = (35, 21)
    script = W.standard_script()
    for sc in script:
        sc.ids = tuple((2, 3, 3)[c] for c in sc.comps) if sc.ss == 0 else (3, 2, 2)[sc.comps[0]]
    blob, route, rec = device(size, 1, noise(size, 1, seed=41), script, 10, 4)
    assert {k for s in rec["scans"] for k in s["tables"]} == {(0, 2), (0, 3), (1, 2), (1, 3)}
    return blob, route, rec


@case("huff_16bit_444")
def _huff_16bit():
    """Every code of every table 16 bits long: the EOBn symbols and the refinement symbols too."""
    size = (40, 24)
    coefs = noise(size, 0, seed=42)
    coefs[1][:, 1:] = 0                                    # a long EOB run as well
    _, recs = W.write_progressive_jpeg(*size, 0, coefs, ONES, W.standard_script())
    script = W.standard_script()
    for sc, r in zip(script, recs):
        tabs = {k: W.table_with_lengths([(s, 16) for s in sorted(r["symbols"][k])]) for k in r["tables"]}
        if sc.ss == 0 and sc.ah == 0:
            sc.tables = [tabs[(0, (0, 1, 1)[c])] for c in sc.comps]
        elif sc.ss:
            sc.tables = tabs[(1, (0, 1, 1)[sc.comps[0]])]
    blob, route, rec = device(size, 0, coefs, script, 10, 4)
    for s in rec["scans"]:
        for k, lengths in s["lengths"].items():
            assert set(lengths) == {16}, (s["kind"], k)
    assert 3 in categories(rec["scans"])
    return blob, route, rec


@case("huff_eob_only_and_one_symbol_dc_h2v2")
def _huff_small_tables():
    """Cb has no AC at all: the table of its AC scan holds one EOBn symbol.  Its DC values are 0 and 1 and its first DC
    scan, on its own at Al = 1, sends differences of 0 only: a DC table of one symbol."""
    size = (35, 21)
    coefs = noise(size, 2, seed=43)
    coefs[1][:, 1:] = 0
    coefs[1][:, 0] = np.arange(len(coefs[1])) % 2
    blob, route, rec = device(size, 2, coefs, simple_script([(0, 2), (1,)], al_dc=1), 7, 2)
    dc, ac = rec["scans"][1], rec["scans"][3]
    assert dc["comps"] == ac["comps"] == (1,)
    assert dc["tables"][(0, 1)] == ([1] + [0] * 15, b"\x00")
    assert ac["tables"][(1, 1)] == ([1] + [0] * 15, b"\x20") and ac["eob_runs"] == [(2, 6)]
    return blob, route, rec


# ------------------------------------------------------------------------------------------------------------
# frames: the component's own raster against the MCU-padded coefficient array
# ------------------------------------------------------------------------------------------------------------
def _size_case(size, sampling):
    def fn():
        coefs = noise(size, sampling, seed=sum(size) + sampling)
        blob, route, rec = device(size, sampling, coefs, simple_script([(0,), (1,), (2,)], al_dc=1), 9, 2)
        assert all(len(s["comps"]) == 1 for s in rec["scans"])
        return blob, route, rec
    return fn


for _s in (0, 1, 2):
    for _tag, _size in (("1xN", (1, 37)), ("Nx1", (37, 1)), ("8k1", (33, 25)), ("3xN", (3, 21)), ("4xN", (4, 21)),
                        ("5xN", (5, 21))):
        case(f"size_{_tag}_{SAMPLING_NAMES[_s]}")(_size_case(_size, _s))


# ------------------------------------------------------------------------------------------------------------
# host by design
# ------------------------------------------------------------------------------------------------------------
SMALL = (40, 32)


@case("host_refine_size2")
def _host_refine_size2():
    coefs = noise(SMALL, 0, seed=50)
    coefs[0][5, 1:] = 0
    coefs[0][5, 3] = 1
    script = simple_script([(0, 1, 2)])
    script[1] = Scan((0,), 1, 63, 0, 1)
    script.append(Scan((0,), 1, 63, 1, 0, symbols={5: [(0x22, 1)]}, strict=False))
    blob, route, rec = host(SMALL, 0, coefs, script, 5, "status", "an AC refinement symbol of size 2: libjpeg warns "
                            "(JWRN_HUFF_BAD_CODE) and reads on, prog_ac_refine returns false and sets kErrDecode")
    assert rec["scans"][4]["symbols"][(1, 0)][0x22] == 1
    return blob, route, rec


@case("host_run_past_se")
def _host_run_past_se():
    coefs = noise(SMALL, 0, seed=51)
    script = [Scan((0, 1, 2), 0, 0, 0, 0), Scan((0,), 1, 5, 0, 0, symbols={7: [(0x71, 1)]}, strict=False),
              Scan((0,), 6, 63, 0, 0), Scan((1,), 1, 63, 0, 0), Scan((2,), 1, 63, 0, 0)]
    blob, route, rec = host(SMALL, 0, coefs, script, 5, "status", "run 7 from coefficient 1 in the band 1..5 lands on "
                            "coefficient 8: libjpeg writes it, prog_ac_first returns false and sets kErrDecode")
    assert rec["scans"][1]["symbols"][(1, 0)][0x71] == 1
    return blob, route, rec


@case("host_no_ac_scans")
def _host_no_ac():
    return host(SMALL, 0, noise(SMALL, 0, seed=52), [Scan((0,), 0, 0, 0, 0), Scan((1, 2), 0, 0, 0, 0)], 2, "parser",
                "DC scans only: libjpeg smooths across blocks", "incomplete scan script")


@case("host_missing_last_refinement")
def _host_missing_refinement():
    return host(SMALL, 0, noise(SMALL, 0, seed=53), W.standard_script()[:-1], 9, "parser",
                "the standard script without its last scan: luma AC stays at Al = 1", "incomplete scan script")


@case("host_65_scans")
def _host_65():
    size = (24, 16)
    return host(size, 0, noise(size, 0, seed=28, amp=3, density=0.6), many_scans(True), 65, "parser",
                "one scan more than MAX_SCANS", "more than 64 scans")


@case("host_ac_before_dc")
def _host_ac_before_dc():
    script = simple_script([(0, 1, 2)])
    script = [script[1], script[0]] + script[2:]
    return host(SMALL, 0, noise(SMALL, 0, seed=54), script, 4, "parser", "libjpeg warns about the progression",
                "AC scan before DC")


@case("host_ah_mismatch")
def _host_ah_mismatch():
    script = simple_script([(0, 1, 2)])
    script[1] = Scan((0,), 1, 63, 0, 2)
    script.append(Scan((0,), 1, 63, 1, 0))
    return host(SMALL, 0, noise(SMALL, 0, seed=55), script, 5, "parser", "a refinement with Ah = 1 behind a first "
                "scan with Al = 2", "bogus progression: Ah does not continue the previous scan")
