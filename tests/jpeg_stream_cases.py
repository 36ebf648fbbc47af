"""Baseline JPEG streams no Pillow save produces, written with tests/jpeg_writer.py: odd Huffman tables, every symbol,
restart layouts, byte layouts around the classifier's lane (16 bytes) and tile (4096 bytes) boundaries, header
variants and a periodic stream that never self-synchronises.  `build(name)` → (blob, expected route, record); every
case asserts from the record or the bytes that it still reaches what it was built for.

Expected route: "device" (decoded on the GPU, Pillow never asked) for every legal stream but the few below, which are
"host" by design; each states its reason in record["why_host"] and whether the parser ("parser") or the device's status
("status") hands it over in record["host_by"]:

    run_past_63      a zero run that passes coefficient 63: libjpeg overwrites coefficient 63, write_span() reports it
    dc_overflow      a running DC that leaves int16: libjpeg wraps it into a short, jpeg_dc_kernel raises kErrRange
    layout_fill      0xFF fill bytes in front of RST markers and EOI: the byte classifier takes 0xFF 0xFF as an error
    header_adobe0    Adobe transform 0: jpeg._frame, "ycc = w.adobe_transform == 1 ... raise _Bad('not YCbCr')"

The AC symbol 0x50 (run 5, size 0) is a "device" case: step() ends the block there, exactly as libjpeg's decode_mcu
("if (r != 15) break") does, so the device's coefficients are libjpeg's and no error bit is raised.
"""
import functools

import numpy as np

import jpeg_writer as W
from test_jpeg_host import smooth_rgb

DEVICE, HOST = "device", "host"
CASES = {}                                                 # name → function returning (blob, route, record)
SAMPLING_NAMES = ("444", "h2v1", "h2v2")


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
    return blob, route, rec


def names(route=None):
    return [n for n in CASES if route is None or build(n)[1] == route]


# ------------------------------------------------------------------------------------------------------------
# building blocks
# ------------------------------------------------------------------------------------------------------------
def ramp_q(lo=2, step=2):
    """A quantisation table in natural order that grows with frequency: lo + step (row + column)."""
    r, c = np.mgrid[0:8, 0:8]
    return (lo + step * (r + c)).reshape(64).astype(np.int64)


FINE, COARSE = ramp_q(2, 1), ramp_q(6, 4)
Q3 = [FINE, FINE, FINE]


def finish(blob, rec, size, sampling, coefs, raw=None, **more):
    """The record every case returns: the writer's, plus the frame and the coefficients that went in (scan order,
    natural order inside a block, DC as a difference: what test_jpeg_host.model_coefficients reads back)."""
    rec = dict(rec, size=size, sampling=sampling, **more)
    rec["coefs"] = W.interleave_natural(coefs, sampling, raw) if coefs is not None else None
    return blob, rec


def picture(size, sampling, q=None, restart=0, seed=0, **kw):
    """A smooth picture of `size` (w, h) through the writer → (blob, record)."""
    q = q or Q3
    w, h = size
    coefs = W.coefficients_from_pixels(smooth_rgb(h, w, seed=seed), sampling, q, restart)
    blob, rec = W.write_jpeg(w, h, sampling, coefs, q, restart=restart, **kw)
    return finish(blob, rec, size, sampling, coefs)


def symbol_stats(coefs):
    """Per component: (Counter of DC categories, Counter of AC symbols) of the blocks as `block_symbols` codes them."""
    out = []
    for blocks in coefs:
        dc, ac = W.Counter(), W.Counter()
        for b in blocks:
            syms = W.block_symbols(b)
            dc[syms[0][0]] += 1
            ac.update(s for s, _ in syms[1:])
        out.append((dc, ac))
    return out


DC_ALPHABET = list(range(12))
AC_ALPHABET = sorted(W.REGULAR_AC | {W.ZRL, W.EOB})


def ranked(alphabet, freq):
    return sorted(alphabet, key=lambda s: (-freq[s], s))


def shaped_table(shape, alphabet, freq):
    """One Huffman table of a prescribed shape over `alphabet`, the symbols the stream uses most getting the codes that
    make the shape show (freq: Counter of the stream's symbols)."""
    r = ranked(alphabet, freq)
    if shape == "all16":                                   # every code 16 bits long: nothing in the lookup table
        return W.table_with_lengths([(s, 16) for s in r])
    if shape == "long":                                    # lengths 10..16 only, the likeliest symbols at 10 and 16
        return W.table_with_lengths([(s, (10, 16, 11, 15, 12, 14, 13)[i % 7]) for i, s in enumerate(r)])
    if shape == "one16":                                   # lengths 1 and 16 only
        return W.table_with_lengths([(r[0], 1)] + [(s, 16) for s in r[1:]])
    if shape == "nine10":                                  # lengths 9 and 10 only: the two sides of kLutBits
        return W.table_with_lengths([(s, 9 + i % 2) for i, s in enumerate(r)])
    if shape == "fffe":
        # one code of every length up to n, then 16-bit codes from there up to 0xFFFE, the last of them a symbol the
        # stream uses: the code next to the reserved all-ones prefix
        if len(alphabet) == 12:                            # DC: 16 symbols (categories 12..15 never occur) at 1..16
            order = [s for s in r if s != r[1]] + [12, 13, 14, 15]
            return W.table_with_lengths([(s, i + 1) for i, s in enumerate(order)] + [(r[1], 16)])
        short = [(s, i + 1) for i, s in enumerate(r[:9])]
        at16 = r[10:10 + 126] + [r[9]]                     # 0xFF80 .. 0xFFFE
        return W.table_with_lengths(short + [(s, 16) for s in at16])
    raise ValueError(shape)


def emitted_lengths(rec, key):
    return {n for n, cnt in rec["lengths"][key].items() if cnt}


# ------------------------------------------------------------------------------------------------------------
# Huffman table shapes
# ------------------------------------------------------------------------------------------------------------
WANT_LENGTHS = {"all16": lambda ls: ls == {16}, "long": lambda ls: {10, 16} <= ls <= set(range(10, 17)),
                "one16": lambda ls: ls == {1, 16}, "nine10": lambda ls: ls == {9, 10},
                "fffe": lambda ls: 16 in ls and 1 in ls}


def _shape_case(shape, sampling):
    def fn():
        size = (43, 29)
        coefs = W.coefficients_from_pixels(smooth_rgb(size[1], size[0], seed=sampling), sampling, Q3)
        stats = symbol_stats(coefs)
        dcs = [shaped_table(shape, DC_ALPHABET, st[0]) for st in stats]
        acs = [shaped_table(shape, AC_ALPHABET, st[1]) for st in stats]
        lay = W.Layout(dc_ids=(0, 1, 2), ac_ids=(0, 1, 2))          # the table is per component
        blob, rec = W.write_jpeg(*size, sampling, coefs, Q3, dcs, acs, layout=lay)
        for key in rec["lengths"]:
            assert WANT_LENGTHS[shape](emitted_lengths(rec, key)), (shape, key, rec["lengths"][key])
        if shape == "fffe":
            for key, t in zip(("dc0", "dc1", "dc2", "ac0", "ac1", "ac2"), dcs + acs):
                last = [s for s, cl in W.table_codes(t).items() if cl == (0xFFFE, 16)]
                assert len(last) == 1 and rec["symbols"][key][last[0]] > 0, key
        blob, rec = finish(blob, rec, size, sampling, coefs)
        return blob, DEVICE, rec
    return fn


for _shape in WANT_LENGTHS:
    for _s in (0, 1, 2):
        case(f"huff_{_shape}_{SAMPLING_NAMES[_s]}")(_shape_case(_shape, _s))


def _table_case(kind, sampling):
    def fn():
        size = (43, 29)
        coefs = W.coefficients_from_pixels(smooth_rgb(size[1], size[0], seed=3 + sampling), sampling, Q3)
        dcs, acs, lay = list(W.STD_DC), list(W.STD_AC), W.Layout()
        if kind == "onedc":                                # a one-symbol DC table: the single code "0"
            for c in coefs:
                c[:, 0] = 0
            dcs = [W.table_with_lengths([(0, 1)])] * 3
            lay = W.Layout(dc_ids=(0, 0, 0))
        stats = symbol_stats(coefs)
        if kind == "ac256":                                # 256 entries: every byte value is a symbol
            acs = [W.table_from_frequencies({s: st[1][s] for s in range(256)}) for st in stats]
            lay = W.Layout(ac_ids=(0, 1, 2))
        elif kind == "shared":                             # one table id for all components
            dcs = [W.table_from_frequencies(sum((st[0] for st in stats), W.Counter({s: 0 for s in DC_ALPHABET})))] * 3
            acs = [W.table_from_frequencies(sum((st[1] for st in stats), W.Counter({s: 0 for s in AC_ALPHABET})))] * 3
            lay = W.Layout(dc_ids=(0, 0, 0), ac_ids=(0, 0, 0))
        elif kind == "ids23":                              # Cb and Cr name different tables, ids 2 and 3
            dcs = [W.STD_DC_LUMA, W.STD_DC_CHROMA, W.table_from_frequencies({s: stats[2][0][s] for s in DC_ALPHABET})]
            acs = [W.STD_AC_LUMA, W.STD_AC_CHROMA, W.table_from_frequencies({s: stats[2][1][s] for s in AC_ALPHABET})]
            lay = W.Layout(dc_ids=(1, 2, 3), ac_ids=(0, 2, 3), qt_ids=(3, 2, 2))
        blob, rec = W.write_jpeg(*size, sampling, coefs, Q3, dcs, acs, layout=lay)
        if kind == "onedc":
            assert rec["dc_categories"] == {0}
            assert emitted_lengths(rec, "dc0") == {1} and W.table_codes(dcs[0]) == {0: (0, 1)}
        elif kind == "ac256":
            assert all(len(t[1]) == 256 for t in acs) and all(rec["lengths"][f"ac{c}"] for c in range(3))
        elif kind == "shared":
            assert set(rec["lengths"]) == {"dc0", "ac0"}
        else:
            assert set(rec["lengths"]) == {"dc1", "dc2", "dc3", "ac0", "ac2", "ac3"} and dcs[1] != dcs[2]
            assert all(sum(v.values()) > 0 for v in rec["lengths"].values())
        blob, rec = finish(blob, rec, size, sampling, coefs)
        return blob, DEVICE, rec
    return fn


for _kind in ("onedc", "ac256", "shared", "ids23"):
    for _s in (0, 1, 2):
        case(f"huff_{_kind}_{SAMPLING_NAMES[_s]}")(_table_case(_kind, _s))


# ------------------------------------------------------------------------------------------------------------
# symbols
# ------------------------------------------------------------------------------------------------------------
ONES = [np.ones(64, np.int64)] * 3                         # dequantised values are the coefficients: far inside kIdctLimit


@case("symbols_all")
def _symbols_all():
    """Every DC category 0..11 (differences up to ±2047) and every AC symbol a baseline stream can hold, 4:4:4, all
    quantisation entries 1.  Y carries one block per regular (run, size) symbol and the odd blocks; Cb the DC
    categories, each difference followed by its negative so the running DC returns to 0; Cr amplitudes of ±1023."""
    mx, my = 14, 12
    n = mx * my
    y, cb, cr = (np.zeros((n, 64), np.int64) for _ in range(3))
    raw = {}
    b = 0
    for r in range(16):
        for s in range(1, 11):
            v = ((1 << s) - 1) if (r + s) % 2 else (1 << (s - 1))        # both ends of the size's range
            y[b, 1 + r] = v if r % 2 else -v
            b += 1
    # three ZRLs, then run 14 to coefficient 63: the block ends there with no EOB
    raw[(0, b)] = [(0, None), (W.ZRL, None), (W.ZRL, None), (W.ZRL, None), (0xE1, -1)]
    b += 1
    y[b, 1:] = np.where(np.arange(63) % 2, 1, -1)          # dense to 63: no run, no EOB
    b += 1
    y[b, 20] = 5                                           # a ZRL that is needed: run 19 = ZRL + run 3
    b += 1
    assert b <= n                                          # the rest of Y: EOB-only blocks
    k = 0
    for cat in range(12):
        for d in sorted({(1 << cat) - 1, (1 << cat) >> 1}):
            cb[k, 0], cb[k + 1, 0] = d, -d
            k += 2
    assert k <= n
    for j in range(0, 64, 2):
        cr[j, 1 + j % 63], cr[j + 1, 1 + (j + 7) % 63] = 1023, -1023
    coefs = [y, cb, cr]
    blob, rec = W.write_jpeg(mx * 8, my * 8, 0, coefs, ONES, raw_blocks=raw)
    assert rec["dc_categories"] == set(range(12))
    assert rec["ac_symbols"] == W.REGULAR_AC | {W.ZRL, W.EOB} and len(W.REGULAR_AC) == 160
    assert rec["symbols"]["dc1"][11] == 4 and {2047, -2047, 1024, -1024} <= set(cb[:, 0].tolist())
    blob, rec = finish(blob, rec, (mx * 8, my * 8), 0, coefs, raw)
    assert rec["coefs"][(160 * 3), 63] == -1               # the coefficient at 63 behind three ZRLs (block 160 of Y)
    return blob, DEVICE, rec


def _small_odd(raw_or_coefs, why=None, by="status"):
    """A 40 x 32 4:4:4 image of near-empty blocks, one AC table (with a code for 0x50) for all components;
    raw_or_coefs(coefs) edits the coefficients in place or returns raw symbol lists for some blocks."""
    mx, my = 5, 4
    n = mx * my
    coefs = [np.zeros((n, 64), np.int64) for _ in range(3)]
    for c in range(3):
        coefs[c][:, 1] = 3 + c                             # something to see in every block
    raw = raw_or_coefs(coefs) or {}
    ac = W.table_from_frequencies({s: 1 for s in AC_ALPHABET + [0x50]})
    blob, rec = W.write_jpeg(mx * 8, my * 8, 0, coefs, ONES, ac_tables=[ac] * 3, layout=W.Layout(ac_ids=(0, 0, 0)),
                             raw_blocks=raw)
    if why:
        blob, rec = finish(blob, rec, (mx * 8, my * 8), 0, None, why_host=why, host_by=by)
        return blob, HOST, rec
    blob, rec = finish(blob, rec, (mx * 8, my * 8), 0, coefs, raw)
    return blob, DEVICE, rec


@case("symbols_0x50")
def _symbols_0x50():
    """AC symbol 0x50 (run 5, size 0): neither ZRL nor EOB.  libjpeg ends the block there, and so does step()."""
    def edit(coefs):
        return {(0, 3): [(2, 3), (0x01, 1), (0x50, None)], (1, 7): [(0, None), (0x50, None)]}
    blob, route, rec = _small_odd(edit)
    assert rec["symbols"]["ac0"][0x50] == 2
    return blob, route, rec


@case("symbols_run_past_63")
def _symbols_run_past_63():
    def edit(coefs):
        return {(0, 4): [(0, None), (W.ZRL, None), (W.ZRL, None), (W.ZRL, None), (0xF1, 1)]}     # 1 + 48 + 15 = 64
    blob, route, rec = _small_odd(edit, "a zero run passes coefficient 63: libjpeg overwrites coefficient 63 "
                                  "(its natural-order table has 16 spare entries), write_span() raises kErrDecode")
    assert rec["symbols"]["ac0"][0xF1] == 1 and rec["symbols"]["ac0"][W.ZRL] == 3
    return blob, route, rec


@case("symbols_dc_overflow")
def _symbols_dc_overflow():
    def edit(coefs):
        coefs[0][:17, 0] = 2047                            # 17 * 2047 = 34799 > 32767
    blob, route, rec = _small_odd(edit, "the running DC leaves int16: libjpeg wraps it into a short (JCOEF), "
                                  "jpeg_dc_kernel raises kErrRange")
    assert rec["symbols"]["dc0"][11] == 17
    return blob, route, rec


# ------------------------------------------------------------------------------------------------------------
# restart intervals
# ------------------------------------------------------------------------------------------------------------
def _restart_case(size, sampling, restart, intervals, write_dri=None, seed=0):
    def fn():
        w, h = size
        hy, vy = W.LUMA_HV[sampling]
        nmcu = -(-w // (8 * hy)) * -(-h // (8 * vy))
        q = [COARSE] * 3
        coefs = W.coefficients_from_pixels(smooth_rgb(h, w, seed=seed), sampling, q,
                                           restart if 0 < restart < nmcu else 0)
        blob, rec = W.write_jpeg(w, h, sampling, coefs, q, restart=restart, layout=W.Layout(write_dri=write_dri))
        assert rec["n_intervals"] == intervals and len(rec["rst"]) == intervals - 1, (rec["n_intervals"], nmcu)
        assert (b"\xff\xdd\x00\x04" in blob[:rec["blob_scan_offset"]]) == (restart > 0 or bool(write_dri))
        blob, rec = finish(blob, rec, size, sampling, coefs, nmcu=nmcu, restart=restart)
        return blob, DEVICE, rec
    return fn


# interval 1 on 17 x 17 MCUs: 289 intervals cross the RST7 wrap and the 256-interval chunk of the segment kernel
case("restart_1_289_444")(_restart_case((136, 136), 0, 1, 289))
case("restart_1_290_h2v1")(_restart_case((147, 229), 1, 1, 290))              # 10 x 29 MCUs, neither side a multiple
case("restart_1_272_h2v2")(_restart_case((245, 265), 2, 1, 272))              # 16 x 17 MCUs
# more than 256 MCUs and no restart at all: the DC scan carries across its 256-MCU chunks
case("restart_none_289_444")(_restart_case((136, 136), 0, 0, 1, seed=1))
case("restart_none_290_h2v1")(_restart_case((147, 229), 1, 0, 1, seed=1))
case("restart_none_272_h2v2")(_restart_case((245, 265), 2, 0, 1, seed=1))
# 300-MCU intervals over 289 .. 272 MCUs would be none; 100 gives a carry inside an interval and a shorter last one
case("restart_100_289_444")(_restart_case((136, 136), 0, 100, 3, seed=2))
# the last interval shorter than the others (28 = 5 * 5 + 3; 12 = 5 + 5 + 2; 9 = 4 + 4 + 1)
case("restart_short_last_444")(_restart_case((56, 32), 0, 5, 6))
case("restart_short_last_h2v1")(_restart_case((45, 27), 1, 5, 3))
case("restart_short_last_h2v2")(_restart_case((45, 43), 2, 4, 3))
# an interval that spans MCU rows (rows of 7, 3 and 3 MCUs)
case("restart_spans_rows_444")(_restart_case((56, 32), 0, 10, 3))
case("restart_spans_rows_h2v1")(_restart_case((45, 27), 1, 4, 3))
case("restart_spans_rows_h2v2")(_restart_case((45, 43), 2, 5, 2))
# DRI equal to the MCU count and above it: no marker is written; and an explicit DRI of 0
case("restart_dri_equals_mcus")(_restart_case((56, 32), 0, 28, 1))
case("restart_dri_above_mcus")(_restart_case((56, 32), 0, 1000, 1))
case("restart_dri_65535_h2v2")(_restart_case((45, 43), 2, 65535, 1))
case("restart_dri_zero")(_restart_case((56, 32), 0, 0, 1, write_dri=True))


# ------------------------------------------------------------------------------------------------------------
# byte layout: the classifier's 16-byte lanes and 4096-byte tiles
# ------------------------------------------------------------------------------------------------------------
def noise_mcus(n, seed):
    """n 4:4:4 MCUs of noise under an all-ones quantisation table, each its own restart interval (restart = 1, so
    the DC entry is the DC value): amplitudes differ from MCU to MCU, so their coded lengths spread widely."""
    rng = np.random.default_rng(seed)
    amp = rng.integers(2, 24, n)
    coefs = [rng.integers(-amp[:, None], amp[:, None] + 1, (n, 64)) for _ in range(3)]
    return [c.astype(np.int64) for c in coefs]


def _interval_layout(rec):
    """Per restart interval of a restart = 1 stream: (length in bytes, offsets of its stuffed 0xFF inside it)."""
    starts = [0] + [r + 2 for r in rec["rst"]]
    ends = rec["rst"] + [rec["scan_len"]]
    ff = np.asarray(rec["ff00"])
    return [(e - s, [int(x) - s for x in ff[(ff >= s) & (ff < e)]]) for s, e in zip(starts, ends)]


@functools.lru_cache(maxsize=None)
def _tile_boundary_order():
    """With restart = 1 every MCU is an interval of its own: its bytes do not depend on where it stands.  So the order of
    96 noise MCUs is searched in plain arithmetic (fixed seed) until one RST marker and one stuffed pair straddle a tile
    boundary (0xFF at offset 4095 mod 4096); the 16-byte lane boundaries come by themselves and are asserted."""
    n = 96
    coefs = noise_mcus(n, seed=5)
    _, rec = W.write_jpeg(96, 64, 0, coefs, ONES, restart=1)
    lay = _interval_layout(rec)
    length = np.array([x[0] for x in lay])
    assert rec["scan_len"] > 8192
    rng = np.random.default_rng(17)
    for _ in range(200000):
        order = rng.permutation(n)
        start = np.concatenate([[0], np.cumsum(length[order] + 2)[:-1]])
        if not np.any((start[1:] - 2) % 4096 == 4095):
            continue
        if any((start[k] + f) % 4096 == 4095 for k, m in enumerate(order) for f in lay[m][1]):
            return [c[order] for c in coefs]
    raise AssertionError("no order of the MCUs puts a marker and a stuffed pair across a tile boundary")


def _layout_case(**lay):
    def fn():
        coefs = _tile_boundary_order()
        blob, rec = W.write_jpeg(96, 64, 0, coefs, ONES, restart=1, layout=W.Layout(**lay))
        fill = lay.get("fill", {}).get("RST", 0)
        ff, rst = np.asarray(rec["ff00"]), np.asarray(rec["rst"])
        scan = blob[rec["blob_scan_offset"]:]
        assert rec["scan_len"] > 8192
        assert all(scan[i] == 0xFF and scan[i + 1] == 0 for i in ff)
        assert all(scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7 for i in rst)
        if not fill and lay.get("pad_ones", True):         # fill bytes and other pad bits move what lies behind them
            assert np.any(ff % 4096 == 4095) and np.any(ff % 16 == 15)
            assert np.any(rst % 4096 == 4095) and np.any(rst % 16 == 15)
        if not lay.get("pad_ones", True):                  # zero pad bits really occur
            ends = [int(r) - 1 for r in rst] + [rec["scan_len"] - 1]
            assert W.write_jpeg(96, 64, 0, coefs, ONES, restart=1)[0] != blob and any(scan[e] & 1 == 0 for e in ends)
        if lay.get("trailer"):
            assert blob.endswith(b"\xff\xd9" + lay["trailer"])
        if lay.get("fill"):
            assert b"\xff\xff\xd0" in scan and blob.endswith(b"\xff\xff\xd9")
            blob, rec = finish(blob, rec, (96, 64), 0, None, host_by="status",
                               why_host="0xFF fill bytes inside the entropy-coded data: segment_bytes() takes an 0xFF "
                               "followed by 0xFF as an unexpected marker and sets kErrSegment")
            return blob, HOST, rec
        blob, rec = finish(blob, rec, (96, 64), 0, coefs)
        return blob, DEVICE, rec
    return fn


case("layout_tile_boundaries")(_layout_case())
case("layout_zero_pad_bits")(_layout_case(pad_ones=False))
case("layout_bytes_after_eoi")(_layout_case(trailer=b"\x00\xff\xd8junk after the end\xff\xd9\xff"))
case("layout_fill")(_layout_case(fill={"RST": 1, "EOI": 1}))


@case("layout_scan_ends_on_tile")
def _layout_scan_ends_on_tile():
    """The last data byte at offset 4095 mod 4096: 35 of 160 noise MCUs chosen by their lengths so that the scan is a
    whole number of tiles, the EOI being the first bytes of the next one."""
    n, pool = 35, 160
    coefs = noise_mcus(pool, seed=9)
    _, rec = W.write_jpeg(160, 64, 0, coefs, ONES, restart=1)
    length = [x[0] for x in _interval_layout(rec)]
    by_len = sorted(range(pool), key=lambda m: length[m])
    pick = None
    for tiles in (1, 2, 3):
        want = 4096 * tiles - 2 * (n - 1)
        for w0 in range(pool - n + 3):
            base = by_len[w0:w0 + n - 2]
            rest = [m for m in by_len if m not in base]
            need = want - sum(length[m] for m in base)
            seen = {}
            for m in rest:
                if need - length[m] in seen:
                    pick = base + [seen[need - length[m]], m]
                    break
                seen[length[m]] = m
            if pick:
                break
        if pick:
            break
    assert pick is not None and len(set(pick)) == n
    pick = sorted(pick)
    coefs = [c[pick] for c in coefs]
    blob, rec = W.write_jpeg(56, 40, 0, coefs, ONES, restart=1)
    assert rec["scan_len"] % 4096 == 0 and rec["scan_len"] > 0
    blob, rec = finish(blob, rec, (56, 40), 0, coefs)
    return blob, DEVICE, rec


@case("layout_scan_ends_on_lane")
def _layout_scan_ends_on_lane():
    """The last data byte at offset 15 mod 16 (and not on a tile boundary), no restart markers."""
    for seed in range(400):
        coefs = noise_mcus(6, seed)
        coefs = W.to_differences(coefs, 0)
        blob, rec = W.write_jpeg(24, 16, 0, coefs, ONES)
        if rec["scan_len"] % 16 == 0 and rec["scan_len"] % 4096:
            blob, rec = finish(blob, rec, (24, 16), 0, coefs)
            return blob, DEVICE, rec
    raise AssertionError("no seed ends the scan on a lane boundary")


# ------------------------------------------------------------------------------------------------------------
# headers
# ------------------------------------------------------------------------------------------------------------
def _header_case(sampling=2, size=(35, 21), q=None, why=None, **lay):
    def fn():
        layout = W.Layout(**lay)
        blob, rec = picture(size, sampling, q=q, seed=2, layout=layout)
        head = blob[:rec["blob_scan_offset"]]
        if lay.get("fill"):
            assert head.count(b"\xff\xff") >= len(lay["fill"])
        for marker, seg_len in lay.get("extra", ()):
            assert bytes([0xFF, marker, seg_len >> 8, seg_len & 255]) in head
        if lay.get("dht_merged"):
            assert head.count(b"\xff\xc4") == (2 if lay.get("redefine") else 1)
        if why:
            rec = dict(rec, coefs=None, why_host=why, host_by="parser")
            return blob, HOST, rec
        return blob, DEVICE, rec
    return fn


for _style in W.HEADER_STYLES[:5]:
    case(f"header_{_style}")(_header_case(header=_style))
case("header_adobe0")(_header_case(header="adobe0", why="Adobe transform 0 (libjpeg reads the components as RGB): jpeg._frame"
                                   " has `ycc = w.adobe_transform == 1` and raises _Bad('not YCbCr')"))
case("header_sof1")(_header_case(sof=0xC1))
case("header_sof1_adobe1_444")(_header_case(sampling=0, sof=0xC1, header="adobe1"))
case("header_dht_merged")(_header_case(dht_merged=True))
case("header_dqt_merged")(_header_case(dqt_merged=True))
case("header_all_merged_redefined")(_header_case(sampling=1, dht_merged=True, dqt_merged=True, redefine=True))
case("header_redefined")(_header_case(redefine=True))
case("header_tables_after_sof")(_header_case(tables_after_sof=True))
case("header_dqt16_small")(_header_case(dqt16=True))
case("header_dqt16_large")(_header_case(dqt16=True, q=[ramp_q(2, 60), ramp_q(200, 40), ramp_q(300, 1)], qt_ids=(0, 1, 2)))
case("header_three_qtables")(_header_case(sampling=0, q=[ramp_q(2, 1), ramp_q(3, 2), ramp_q(5, 3)], qt_ids=(2, 0, 3)))
case("header_extra_segments")(_header_case(extra=((0xFE, 2), (0xE5, 65535), (0xFE, 65535), (0xE0, 7), (0xEE, 9))))
case("header_fill_bytes")(_header_case(fill={"APP": 1, "DQT": 2, "SOF": 1, "DHT": 3, "SOS": 1}))
case("header_fill_bytes_dri")(lambda: _restart_fill())


def _restart_fill():
    size, q = (35, 21), [COARSE] * 3
    coefs = W.coefficients_from_pixels(smooth_rgb(21, 35, seed=4), 1, q, 2)
    blob, rec = W.write_jpeg(35, 21, 1, coefs, q, restart=2, layout=W.Layout(fill={"DRI": 2, "SOS": 2}))
    assert b"\xff\xff\xff\xdd" in blob and len(rec["rst"]) == 4
    blob, rec = finish(blob, rec, size, 1, coefs)
    return blob, DEVICE, rec


# 3, 4 and 5 pixels wide: libjpeg replicates chroma that is at most two samples wide instead of filtering it (jdsample.c)
for _s in (0, 1, 2):
    _hy, _vy = W.LUMA_HV[_s]
    for _tag, _size in (("1xN", (1, 37)), ("Nx1", (37, 1)), ("8k1", (33, 25)), ("column", (8 * _hy, 43)),
                        ("3xN", (3, 21)), ("4xN", (4, 21)), ("5xN", (5, 21))):
        case(f"size_{_tag}_{SAMPLING_NAMES[_s]}")(_header_case(sampling=_s, size=_size))


# ------------------------------------------------------------------------------------------------------------
# self-synchronisation
# ------------------------------------------------------------------------------------------------------------
@case("sync_periodic")
def _sync_periodic():
    """A stream on which a decoder that starts out of phase stays out of phase.  Both tables give every symbol three
    bits in all (code "0" + 2 amplitude bits, "10" + 1, "110" + 0; "111" unused), the three components share them, and
    every block is DC 0, coefficient 1 = -3, EOB: the nine bits 110 000 110.  Read from bit 1 or 2 of a block, the
    stream is an endless row of valid three-bit symbols (100 001 101 ..., 000 011 011 ...) without a single EOB, so
    such a decoder never errs and never falls into step.  Nine is odd, hence coprime to subseq_bits = 64: the units
    start at every phase 64 u mod 9; one in nine speculates right, two in nine start between symbols of a block and
    fall into step within twelve bits (with the wrong block index), the rest never do.  With one sync pass the interval
    cannot converge, so jpeg_serial_kernel walks it, keeping the units whose recorded start state was exact and
    decoding the others again.  DevicePreprocessor does not report which kernel ran; the pixels must be Pillow's."""
    dc = W.table_with_lengths([(2, 1), (1, 2), (0, 3)])
    ac = W.table_with_lengths([(0x02, 1), (0x01, 2), (W.EOB, 3)])
    mx = my = 8
    n = mx * my
    coefs = [np.zeros((n, 64), np.int64) for _ in range(3)]
    for c in coefs:
        c[:, 1] = -3
    lay = W.Layout(dc_ids=(0, 0, 0), ac_ids=(0, 0, 0))
    blob, rec = W.write_jpeg(mx * 8, my * 8, 0, coefs, Q3, [dc] * 3, [ac] * 3, layout=lay)
    bits = 9 * 3 * n
    assert rec["scan_len"] == -(-bits // 8) and not rec["ff00"]
    scan = blob[rec["blob_scan_offset"]:rec["blob_scan_offset"] + rec["scan_len"]]
    stream = bin(int.from_bytes(scan, "big"))[2:].zfill(8 * len(scan))[:bits]
    assert stream == "110000110" * (3 * n)
    for phase in (1, 2):                                   # out of phase: valid symbols for ever, never an EOB
        cells = {stream[i:i + 3] for i in range(phase, bits - 3, 3)}
        assert cells and not cells & {"110", "111"}
    assert bits > 20 * 64                                  # many units of 64 bits in the one interval
    blob, rec = finish(blob, rec, (mx * 8, my * 8), 0, coefs)
    return blob, DEVICE, rec
