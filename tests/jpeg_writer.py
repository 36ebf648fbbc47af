"""A baseline JPEG writer for the tests: plain Python and numpy, no encoder behind it.

The input is quantised coefficients, not pixels, and the writer emits exactly the symbols it is told to emit, under
whatever Huffman tables and marker layout the caller names.  It never needs to agree with any encoder: Pillow decodes
the same bytes and is the oracle for what they mean.  `write_jpeg` returns the file and a record of what went into the
scan (code lengths used per table, DC categories and AC symbols emitted, where the stuffed 0xFF00 pairs and the RST
markers lie, the scan's length), from which a test case asserts that it still reaches what it was built to reach.
`write_progressive_jpeg` does the same for an SOF2 file and a scan script (ITU-T T.81 G.1.2), with one record per scan;
its coefficients carry the DC value, not the difference.

Conventions
    sampling     0: 4:4:4, 1: 4:2:2 (h2v1), 2: 4:2:0 (h2v2), as jpeg.SAMPLING
    coefs        three int arrays [n_blocks, 64], one per component, blocks in MCU order (the luma blocks of an MCU
                 consecutive, row-major inside it), each block in ZIG-ZAG order; entry 0 is the DC DIFFERENCE that is
                 coded, not the DC value
    qtables      three int arrays [64] in natural (row-major) order, one per component, as jpeg.parse returns them
    huffman      a table is (bits[16], vals): the number of codes of each length 1..16 and the symbols in code order
"""
from __future__ import annotations

import heapq
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from on_device_image_captioning_amd.jpeg import NATURAL_ORDER

LUMA_BLOCKS = (1, 2, 4)
LUMA_HV = ((1, 1), (2, 1), (2, 2))

# the tables of ITU-T T.81 Annex K.3
STD_DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], bytes(range(12)))
STD_DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], bytes(range(12)))
STD_AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
STD_AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
STD_DC = [STD_DC_LUMA, STD_DC_CHROMA, STD_DC_CHROMA]
STD_AC = [STD_AC_LUMA, STD_AC_CHROMA, STD_AC_CHROMA]

#: every regular AC symbol (run 0..15, size 1..10), plus ZRL and EOB: what a baseline 8-bit stream can contain
REGULAR_AC = frozenset((r << 4) | s for r in range(16) for s in range(1, 11))
ZRL, EOB = 0xF0, 0x00

HEADER_STYLES = ("jfif", "adobe1", "bare123", "jfif012", "jfifRGB", "adobe0")


@dataclass
class Layout:
    """Everything about a file that is not the coefficients: markers, their order and their padding."""
    sof: int = 0xC0                      # 0xC0 (SOF0) or 0xC1 (SOF1)
    header: str = "jfif"                 # one of HEADER_STYLES: jfif (ids 1, 2, 3) | adobe1 (APP14 transform 1, no JFIF)
                                         # | bare123 (neither, ids 1, 2, 3) | jfif012 | jfifRGB (ids 'R', 'G', 'B')
                                         # | adobe0 (APP14 transform 0: libjpeg takes the components as RGB)
    dht_merged: bool = False             # one DHT segment for all tables instead of one each
    dqt_merged: bool = False             # the same for DQT
    dqt16: bool = False                  # 16-bit DQT entries (Pq = 1)
    redefine: bool = False               # every table is defined twice; the later definition is the one given
    tables_after_sof: bool = False       # DQT behind the SOF (DHT always is)
    qt_ids: tuple = (0, 1, 1)            # table id 0..3 each component names; components that share an id share a table
    dc_ids: tuple = (0, 1, 1)
    ac_ids: tuple = (0, 1, 1)
    extra: tuple = ()                    # ((marker byte, segment length incl. its two length bytes), ...): COM / APPn
    fill: dict = field(default_factory=dict)   # extra 0xFF bytes in front of "APP", "DQT", "SOF", "DHT", "DRI", "SOS",
                                               # "RST", "EOI": name → count
    write_dri: object = None             # None: a DRI segment iff restart > 0; True: always (an explicit DRI of 0)
    pad_ones: bool = True                # the bits that complete the last byte of an interval
    trailer: bytes = b""                 # bytes after the EOI


# ------------------------------------------------------------------------------------------------------------
# Huffman tables
# ------------------------------------------------------------------------------------------------------------
def check_table(table):
    """Raise ValueError for a table libjpeg's jdhuff.c (jpeg_make_d_derived_tbl) refuses: more than 256 symbols, or
    codes that overflow the code space — the all-ones code of any length counts as overflow."""
    bits, vals = table
    if len(bits) != 16 or sum(bits) != len(vals) or not 1 <= len(vals) <= 256:
        raise ValueError("bits and vals do not describe one table")
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code >= (1 << length):
            raise ValueError(f"Huffman code space overflows at length {length}")
        code <<= 1


def table_codes(table):
    """symbol → (code, length), the canonical assignment of ITU-T T.81 Annex C."""
    check_table(table)
    bits, vals = table
    out, code, p = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out.setdefault(vals[p], (code, length))
            code += 1
            p += 1
        code <<= 1
    return out


def table_with_lengths(lengths):
    """A table with prescribed code lengths.  lengths: [(symbol, length)] or {symbol: length}; symbols of one length
    get their codes in the order given.  Refused (ValueError) where the code space overflows."""
    items = list(lengths.items()) if isinstance(lengths, dict) else list(lengths)
    bits = [0] * 16
    for _, length in items:
        if not 1 <= length <= 16:
            raise ValueError("code lengths are 1..16")
        bits[length - 1] += 1
    vals = bytes(s for length in range(1, 17) for s, ln in items if ln == length)
    table = (bits, vals)
    check_table(table)
    return table


def table_from_frequencies(freq, max_len=16):
    """A Huffman table for {symbol: count} (every symbol named gets a code, a count of 0 included) with no code
    longer than max_len and the all-ones code left free: Huffman's algorithm with a reserved symbol of the lowest
    weight, then the length-limiting adjustment of ITU-T T.81 K.2 (Figure K.3)."""
    syms = sorted(freq)
    if not syms:
        raise ValueError("no symbols")
    heap = [(max(freq[s], 0) + 1, s, [s]) for s in syms] + [(0, 256, [256])]      # 256: reserves the all-ones code
    heapq.heapify(heap)
    depth = Counter()
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]), a[2] + b[2]))
    bits = [0] * (max(depth.values()) + 1)
    for s in depth:
        bits[depth[s]] += 1
    for i in range(len(bits) - 1, max_len, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    bits = (bits + [0] * 17)[:max_len + 1]
    i = max_len
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                   # the reserved symbol holds the longest code
    order = sorted(syms, key=lambda s: (depth[s], -freq[s], s))    # code order: by length, likelier first
    table = ((bits[1:] + [0] * 16)[:16], bytes(order))
    check_table(table)
    return table


# ------------------------------------------------------------------------------------------------------------
# entropy coding
# ------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def flush(self, ones):
        if self.n:
            pad = 8 - self.n
            self.put(((1 << pad) - 1) if ones else 0, pad)


def amplitude_bits(value, size):
    """The `size` bits that follow a symbol for `value` (T.81 F.1.2.1: a negative value is sent as value - 1)."""
    return (value if value >= 0 else value + (1 << size) - 1) & ((1 << size) - 1)


def block_symbols(block):
    """The symbols a well-behaved encoder writes for one zig-zag block whose entry 0 is the DC difference:
    [(symbol, value or None)], the first for the DC table, the rest for the AC table.  Runs of 16 zeros become
    ZRLs; an EOB closes the block unless coefficient 63 is nonzero."""
    d = int(block[0])
    out = [(abs(d).bit_length(), d if d else None)]
    run = 0
    for k in range(1, 64):
        v = int(block[k])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append((ZRL, None))
            run -= 16
        out.append(((run << 4) | abs(v).bit_length(), v))
        run = 0
    if run:
        out.append((EOB, None))
    return out


def symbols_block(symbols):
    """The zig-zag block (DC as its difference) libjpeg reads from a symbol list that stays inside the block; the
    inverse of `block_symbols` for lists that encoder could have written."""
    block = np.zeros(64, np.int64)
    block[0] = symbols[0][1] or 0
    k = 1
    for sym, value in symbols[1:]:
        r, s = sym >> 4, sym & 15
        if s:
            k += r
            block[k] = value
            k += 1
        elif r == 15:
            k += 16
        else:
            break
    return block


# ------------------------------------------------------------------------------------------------------------
# marker emission, shared by the baseline and the progressive writer
# ------------------------------------------------------------------------------------------------------------
def _segment(out, lay, name, marker, payload):
    if len(payload) + 2 > 65535:
        raise ValueError("segment too long")
    out.extend(b"\xff" * lay.fill.get(name, 0))
    out.extend(bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]))
    out.extend(payload)


def _tables(out, lay, name, marker, defs, payload, merged, decoy):
    rounds = [[payload(lay, k, decoy(t)) for k, t in defs]] if lay.redefine else []
    rounds.append([payload(lay, k, t) for k, t in defs])
    for parts in rounds:
        if merged:
            _segment(out, lay, name, marker, b"".join(parts))
        else:
            for p in parts:
                _segment(out, lay, name, marker, p)


def _dqt_payload(lay, i, t):
    zz = [t[NATURAL_ORDER[k]] for k in range(64)]
    if lay.dqt16:
        return bytes([0x10 | i]) + b"".join(bytes([v >> 8, v & 255]) for v in zz)
    return bytes([i]) + bytes(zz)


def _dht_payload(lay, key, t):
    return bytes([(key[0] << 4) | key[1]]) + bytes(t[0]) + bytes(t[1])


def _decoy_dht(t):                                      # another legal table: the same lengths, the symbols reversed
    return (t[0], bytes(reversed(t[1])))


def _prologue(out, lay, sof_marker, width, height, hy, vy, qt):
    """APPn / COM, DQT and the SOF of a three-component frame behind the SOI → the component ids of the frame."""
    def emit_dqt():
        _tables(out, lay, "DQT", 0xDB, sorted(qt.items()), _dqt_payload, lay.dqt_merged,
                lambda t: [min(v + 3, 255) for v in t])

    jfif = b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
    if lay.header.startswith("jfif"):
        _segment(out, lay, "APP", 0xE0, jfif)
    elif lay.header.startswith("adobe"):
        _segment(out, lay, "APP", 0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([int(lay.header[-1])]))
    ids = {"jfif012": (0, 1, 2), "jfifRGB": (ord("R"), ord("G"), ord("B"))}.get(lay.header, (1, 2, 3))
    for marker, seg_len in lay.extra:
        if not (0xE0 <= marker <= 0xEF or marker == 0xFE) or seg_len < 2:
            raise ValueError("extra segments are APPn or COM, of length 2 or more")
        _segment(out, lay, "APP", marker, bytes((7 * k + marker) & 0x7F for k in range(seg_len - 2)))
    if not lay.tables_after_sof:
        emit_dqt()
    sof = bytes([8, height >> 8, height & 255, width >> 8, width & 255, 3])
    for c in range(3):
        sof += bytes([ids[c], (hy << 4) | vy if c == 0 else 0x11, lay.qt_ids[c]])
    _segment(out, lay, "SOF", sof_marker, sof)
    if lay.tables_after_sof:
        emit_dqt()
    return ids


def write_jpeg(width, height, sampling, coefs, qtables, dc_tables=None, ac_tables=None, restart=0, layout=None,
               raw_blocks=None):
    """One baseline file → (bytes, record).

    dc_tables / ac_tables: one table per component (default: the standard ones).  restart: the restart interval in
    MCUs that goes into the DRI segment; markers are written between intervals, so a value at or above the MCU count
    writes none.  raw_blocks: {(component, block index within the component): [(symbol, value or None), ...]}: that
    block is written from the list as it stands (first entry through the DC table; the amplitude takes symbol & 15
    bits) and its row in `coefs` is ignored.

    record: dict with
        lengths      {"dc<id>" / "ac<id>": Counter {code length: times emitted}}
        symbols      {"dc<id>" / "ac<id>": Counter {symbol: times emitted}}
        dc_categories, ac_symbols   sets of what was emitted
        ff00, rst    byte offsets, from the first scan byte, of the 0xFF of every stuffed pair / of every RST marker
        scan_len     bytes of entropy-coded data: from the first scan byte up to the fill bytes or the EOI
        n_intervals  restart intervals written
        blob_scan_offset   where the scan starts in the file
    """
    lay = layout or Layout()
    dc_tables = list(dc_tables or STD_DC)
    ac_tables = list(ac_tables or STD_AC)
    raw_blocks = raw_blocks or {}
    if lay.header not in HEADER_STYLES or lay.sof not in (0xC0, 0xC1):
        raise ValueError("unknown header style or SOF")
    hy, vy = LUMA_HV[sampling]
    nY = hy * vy
    mcus_x, mcus_y = -(-width // (8 * hy)), -(-height // (8 * vy))
    nmcu = mcus_x * mcus_y
    coefs = [np.asarray(c) for c in coefs]
    for c, per in zip(coefs, (nY, 1, 1)):
        if c.shape != (nmcu * per, 64):
            raise ValueError(f"component has {c.shape} coefficients, the frame needs {(nmcu * per, 64)}")

    def shared(ids, tables, what):
        by_id = {}
        for i, t in zip(ids, tables):
            if not 0 <= i <= 3:
                raise ValueError("table ids are 0..3")
            t = (list(t[0]), bytes(t[1])) if what != "qt" else [int(x) for x in t]
            if by_id.setdefault(i, t) != t:
                raise ValueError(f"components share {what} id {i} but not the table")
        return by_id

    qt = shared(lay.qt_ids, qtables, "qt")
    dht = {(0, i): t for i, t in shared(lay.dc_ids, dc_tables, "dc").items()}
    dht.update({(1, i): t for i, t in shared(lay.ac_ids, ac_tables, "ac").items()})
    for t in dht.values():
        check_table(t)
    for t in qt.values():
        if len(t) != 64 or min(t) < 1 or max(t) > (65535 if lay.dqt16 else 255):
            raise ValueError("quantisation entries do not fit the DQT precision")
    codes = {key: table_codes(t) for key, t in dht.items()}

    # ---- the scan
    rec = dict(lengths={f"{'da'[tc]}c{i}": Counter() for tc, i in dht},
               symbols={f"{'da'[tc]}c{i}": Counter() for tc, i in dht}, dc_categories=set(), ac_symbols=set(),
               ff00=[], rst=[])
    comp_of = [0] * nY + [1, 2]
    R = restart if 0 < restart < nmcu else nmcu
    scan = bytearray()
    n_int = 0
    for m0 in range(0, nmcu, R):
        if m0:
            scan += b"\xff" * lay.fill.get("RST", 0)
            rec["rst"].append(len(scan))
            scan += bytes([0xFF, 0xD0 + (n_int - 1) % 8])
        bw = _Bits()
        for m in range(m0, min(m0 + R, nmcu)):
            for j, c in enumerate(comp_of):
                b = m * nY + j if c == 0 else m
                syms = raw_blocks.get((c, b))
                if syms is None:
                    syms = block_symbols(coefs[c][b])
                for n, (sym, value) in enumerate(syms):
                    tc, name = (0, "dc") if n == 0 else (1, "ac")
                    tid = (lay.dc_ids if n == 0 else lay.ac_ids)[c]
                    if sym not in codes[(tc, tid)]:
                        raise ValueError(f"{name} table {tid} has no code for symbol {sym:#04x}")
                    code, length = codes[(tc, tid)][sym]
                    bw.put(code, length)
                    rec["lengths"][f"{name}{tid}"][length] += 1
                    rec["symbols"][f"{name}{tid}"][sym] += 1
                    (rec["dc_categories"] if n == 0 else rec["ac_symbols"]).add(sym)
                    size = sym & 15
                    if size:
                        if value is None or abs(value).bit_length() > size:
                            raise ValueError(f"value {value} does not fit symbol {sym:#04x}")
                        bw.put(amplitude_bits(value, size), size)
        bw.flush(lay.pad_ones)
        base = len(scan)
        rec["ff00"] += [base + i for i, x in enumerate(bw.out) if x == 0xFF]
        scan += bw.out
        n_int += 1
    rec["scan_len"], rec["n_intervals"] = len(scan), n_int

    # ---- the headers
    out = bytearray(b"\xff\xd8")
    ids = _prologue(out, lay, lay.sof, width, height, hy, vy, qt)

    def segment(name, marker, payload):
        _segment(out, lay, name, marker, payload)

    _tables(out, lay, "DHT", 0xC4, sorted(dht.items()), _dht_payload, lay.dht_merged, _decoy_dht)
    if lay.write_dri or (lay.write_dri is None and restart > 0):
        if not 0 <= restart <= 65535:
            raise ValueError("restart interval does not fit the DRI segment")
        segment("DRI", 0xDD, bytes([restart >> 8, restart & 255]))
    sos = bytes([3])
    for c in range(3):
        sos += bytes([ids[c], (lay.dc_ids[c] << 4) | lay.ac_ids[c]])
    segment("SOS", 0xDA, sos + b"\x00\x3f\x00")
    rec["blob_scan_offset"] = len(out)
    out += scan
    out += b"\xff" * lay.fill.get("EOI", 0) + b"\xff\xd9" + lay.trailer
    return bytes(out), rec


# ------------------------------------------------------------------------------------------------------------
# the progressive writer: the four coding procedures of ITU-T T.81 G.1.2
# ------------------------------------------------------------------------------------------------------------
@dataclass
class Scan:
    """One scan of a progressive script.

    comps     frame component indices (0: Y, 1: Cb, 2: Cr) in frame order; an AC scan (ss > 0) names one
    restart   the DRI value in effect, in the scan's own units (MCUs of an interleaved scan, else blocks of the
              component's own raster); markers go between intervals, so a value at or above the unit count writes none
    tables    None: optimal tables from this scan's own symbol counts.  A first DC scan: one table per component of the
              scan; an AC scan: one table.  DC refinement scans use none
    ids       the table ids (0..3) the SOS names: one per component (DC) or one int (AC); default (0, 1, 1)[component]
    symbols   AC scans: {block ordinal in the scan: [(symbol, value), ...]}: the block is written from the list instead of
              what an encoder would choose.  (r << 4 | s, value) with s > 0 codes `value` behind r zeros (refinement:
              behind r still-zero coefficients; a sign bit follows whatever s is), (ZRL, None) sixteen zeros, and
              (r << 4, n) with r < 15 an EOBr that announces a run of n blocks, this one included, whether or not so many
              remain.  A list that ends inside the band without an EOBr joins the encoder's own EOB run
    cut       block ordinals in front of which the pending EOB run is flushed, so that runs come out shorter
    strict    the symbol lists must code exactly the coefficients given; False for streams that are wrong on purpose
    """
    comps: tuple
    ss: int
    se: int
    ah: int
    al: int
    restart: int = 0
    tables: object = None
    ids: object = None
    symbols: dict = field(default_factory=dict)
    cut: tuple = ()
    strict: bool = True


def component_raster(width, height, sampling, c):
    """(blocks per row, block rows) of component c's own raster: what a non-interleaved scan walks (T.81 A.2.2)."""
    hy, vy = LUMA_HV[sampling]
    h, v = (hy, vy) if c == 0 else (1, 1)
    return -(-(-(-width * h // hy)) // 8), -(-(-(-height * v // vy)) // 8)


def raster_to_mcu_order(width, height, sampling, c):
    """For every block of component c's own raster, row by row: its index in the component's MCU-ordered array."""
    hy, vy = LUMA_HV[sampling]
    hh, vv = (hy, vy) if c == 0 else (1, 1)
    mcus_x = -(-width // (8 * hy))
    bw, bh = component_raster(width, height, sampling, c)
    by, bx = np.mgrid[0:bh, 0:bw]
    return (((by // vv) * mcus_x + bx // hh) * (hh * vv) + (by % vv) * hh + bx % hh).reshape(-1)


class _ScanCoder:
    """Turns one scan into tokens: ("s", table key, symbol), ("b", value, bits), ("c", [correction bits]), ("r",)."""

    def __init__(self, sc, width, height, sampling, coefs):
        self.sc, self.tok = sc, []
        self.eob_runs, self.zrl = [], 0
        nY = LUMA_BLOCKS[sampling]
        hy, vy = LUMA_HV[sampling]
        nmcu = -(-width // (8 * hy)) * -(-height // (8 * vy))
        if len(sc.comps) > 1:
            self.n_units = nmcu
            self.unit_blocks = None
        else:
            self.order = raster_to_mcu_order(width, height, sampling, sc.comps[0])
            self.n_units = len(self.order)
        self.R = sc.restart if 0 < sc.restart < self.n_units else self.n_units
        ids = sc.ids
        if sc.ss == 0:
            ids = tuple(ids) if ids is not None else tuple((0, 1, 1)[c] for c in sc.comps)
            self.keys = {c: (0, i) for c, i in zip(sc.comps, ids)}
        else:
            self.key = (1, ids if ids is not None else (0, 1, 1)[sc.comps[0]])
        for k0 in range(0, self.n_units, self.R):
            if k0:
                self.tok.append(("r",))
            units = range(k0, min(k0 + self.R, self.n_units))
            if sc.ss == 0:
                blocks = []
                for u in units:
                    if len(sc.comps) == 1:
                        blocks.append((sc.comps[0], int(self.order[u])))
                    else:
                        for c in sc.comps:
                            per = nY if c == 0 else 1
                            blocks += [(c, u * per + j) for j in range(per)]
                (self.dc_first if sc.ah == 0 else self.dc_refine)(blocks, coefs)
            else:
                (self.ac_first if sc.ah == 0 else self.ac_refine)(units, coefs[sc.comps[0]])

    # G.1.2.1
    def dc_first(self, blocks, coefs):
        pred = {c: 0 for c in self.sc.comps}
        for c, b in blocks:
            v = int(coefs[c][b][0]) >> self.sc.al               # the point transform of DC is an arithmetic shift
            d, pred[c] = v - pred[c], v
            cat = abs(d).bit_length()
            self.tok.append(("s", self.keys[c], cat))
            if cat:
                self.tok.append(("b", amplitude_bits(d, cat), cat))

    def dc_refine(self, blocks, coefs):
        for c, b in blocks:
            self.tok.append(("b", (int(coefs[c][b][0]) >> self.sc.al) & 1, 1))

    # EOB runs, shared by G.1.2.2 and G.1.2.3
    def flush_run(self):
        if self.run:
            r = self.run.bit_length() - 1
            self.eobn(r, self.run)
            if self.be:
                self.tok.append(("c", self.be))
            self.run, self.be = 0, []

    def eobn(self, r, n):
        if not (1 << r) <= n < (2 << r) or r > 14:
            raise ValueError(f"a run of {n} blocks is no EOB{r}")
        self.tok.append(("s", self.key, r << 4))
        if r:
            self.tok.append(("b", n - (1 << r), r))
        self.eob_runs.append((r, n))

    def end_block(self, br):
        self.run += 1
        self.be += br
        if self.run == 0x7FFF:
            self.flush_run()

    # G.1.2.2
    def ac_first(self, units, comp):
        sc = self.sc
        self.run, self.be, forced = 0, [], 0
        band = np.abs(comp[self.order[units.start:units.stop], sc.ss:sc.se + 1]) >> sc.al
        busy = band.any(axis=1)
        for i, n in enumerate(units):
            ops = sc.symbols.get(n)
            if n in sc.cut:
                self.flush_run()
            if forced:                                          # inside a run an explicit EOBn announced
                forced -= 1
                if sc.strict and (busy[i] or ops):
                    raise ValueError(f"block {n} lies inside an announced EOB run but has coefficients")
                continue
            if ops is None and not busy[i]:
                self.end_block([])
                continue
            blk = comp[self.order[n]]
            if ops is None:
                r = 0
                for k in range(sc.ss, sc.se + 1):
                    v = int(blk[k])
                    mag = abs(v) >> sc.al
                    if mag == 0:
                        r += 1
                        continue
                    self.flush_run()
                    while r > 15:
                        self.tok.append(("s", self.key, ZRL))
                        self.zrl += 1
                        r -= 16
                    size = mag.bit_length()
                    self.tok.append(("s", self.key, (r << 4) | size))
                    self.tok.append(("b", amplitude_bits(mag if v > 0 else -mag, size), size))
                    r = 0
                if r:
                    self.end_block([])
                continue
            k, seen = sc.ss, np.zeros(64, np.int64)
            for sym, value in ops:
                r, s = sym >> 4, sym & 15
                self.flush_run()
                if s:
                    k += r
                    self.tok.append(("s", self.key, sym))
                    self.tok.append(("b", amplitude_bits(value, s), s))
                    if k <= 63:
                        seen[k] = value
                    k += 1
                elif r == 15:
                    self.tok.append(("s", self.key, ZRL))
                    self.zrl += 1
                    k += 16
                else:
                    self.eobn(r, value)
                    forced = value - 1
                    k = None
                    break
            if sc.strict:
                want = np.zeros(64, np.int64)
                want[sc.ss:sc.se + 1] = np.sign(blk[sc.ss:sc.se + 1]) * band[i]
                if not np.array_equal(seen, want) or (k is not None and k > sc.se + 1):
                    raise ValueError(f"the symbols of block {n} do not code its coefficients")
            if k is not None and k <= sc.se:
                self.end_block([])
        self.flush_run()

    # G.1.2.3
    def ac_refine(self, units, comp):
        sc = self.sc
        self.run, self.be, forced = 0, [], 0
        band = np.abs(comp[self.order[units.start:units.stop], sc.ss:sc.se + 1]) >> sc.al
        busy = band.any(axis=1)
        for i, n in enumerate(units):
            ops = sc.symbols.get(n)
            if n in sc.cut:
                self.flush_run()
            if ops is None and not busy[i] and not forced:
                self.end_block([])
                continue
            blk = comp[self.order[n]]
            mag = [0] * sc.ss + [int(m) for m in band[i]]       # by zig-zag index; 1: becomes nonzero in this scan
            if forced:                                          # only correction bits, straight behind the EOBn's
                forced -= 1
                if sc.strict and (1 in mag or ops):
                    raise ValueError(f"block {n} lies inside an announced EOB run but has new coefficients")
                self.tok.append(("c", [m & 1 for m in mag if m > 1]))
                continue
            if ops is None:
                new = [k for k in range(sc.ss, sc.se + 1) if mag[k] == 1]
                last_new = new[-1] if new else -1
                r, br = 0, []
                for k in range(sc.ss, sc.se + 1):
                    m = mag[k]
                    if m == 0:
                        r += 1
                        continue
                    while r > 15 and k <= last_new:
                        self.flush_run()
                        self.tok.append(("s", self.key, ZRL))
                        self.tok.append(("c", br))
                        self.zrl += 1
                        r, br = r - 16, []
                    if m > 1:
                        br.append(m & 1)
                        continue
                    self.flush_run()
                    self.tok.append(("s", self.key, (r << 4) | 1))
                    self.tok.append(("b", 1 if blk[k] > 0 else 0, 1))
                    self.tok.append(("c", br))
                    r, br = 0, []
                if r or br:
                    self.end_block(br)
                continue
            k, placed = sc.ss, set()

            def walk(k, r):                                     # past r still-zero coefficients, on to the next one
                bits = []
                while k <= sc.se:
                    if mag[k] > 1:
                        bits.append(mag[k] & 1)
                    else:
                        if sc.strict and mag[k] == 1 and r:
                            raise ValueError(f"block {n}: a run passes over the new coefficient {k}")
                        if r == 0:
                            break
                        r -= 1
                    k += 1
                return k, bits

            for sym, value in ops:
                r, s = sym >> 4, sym & 15
                self.flush_run()
                if s == 0 and r < 15:
                    self.eobn(r, value)
                    forced = value - 1
                    if sc.strict and any(mag[j] == 1 for j in range(k, sc.se + 1)):
                        raise ValueError(f"block {n}: new coefficients behind the EOB")
                    self.tok.append(("c", [mag[j] & 1 for j in range(k, sc.se + 1) if mag[j] > 1]))
                    k = None
                    break
                k, bits = walk(k, r)
                self.tok.append(("s", self.key, sym))
                if s:
                    self.tok.append(("b", 1 if value > 0 else 0, 1))
                    if sc.strict and not (s == 1 and k <= sc.se and mag[k] == 1 and (blk[k] > 0) == (value > 0)):
                        raise ValueError(f"block {n}: no new coefficient of that sign at {k}")
                    placed.add(k)
                else:
                    self.zrl += 1
                self.tok.append(("c", bits))
                k += 1
            if k is not None:
                rest = range(min(k, sc.se + 1), sc.se + 1)
                if sc.strict and any(mag[j] == 1 for j in rest):
                    raise ValueError(f"the symbols of block {n} do not code its coefficients")
                if k <= sc.se:
                    self.end_block([mag[j] & 1 for j in rest if mag[j] > 1])
        self.flush_run()


def write_progressive_jpeg(width, height, sampling, coefs, qtables, script, layout=None):
    """One progressive (SOF2) file → (bytes, [record per scan]).

    coefs: as `write_jpeg`, but entry 0 of a block is the DC VALUE and every entry is the final quantised value: each
    scan sends the part of it that its Ah / Al name.  Blocks of the MCU-ordered arrays that lie outside a component's
    own raster are reached by interleaved scans only.  script: [Scan].  A DHT segment goes in front of a scan for every
    table it names that the id does not hold already, a DRI segment wherever the interval changes.  layout: the
    header fields of `Layout` (header, qt_ids, the DQT options, extra, fill, pad_ones, trailer).

    record (per scan): dict with
        kind         "dc_first" | "dc_refine" | "ac_first" | "ac_refine";  comps, ss, se, ah, al, restart as given
        tables       {(class, id): table} as named by the SOS;  defined: the keys a DHT in front of this scan defines
        lengths, symbols   {(class, id): Counter} of code lengths / symbols emitted
        eob_runs     [(EOBn category, run length)] in emission order;  zrl: ZRLs emitted
        max_correction_bits   the most correction bits behind one symbol
        ff00, rst    offsets from the scan's first data byte, as `write_jpeg`;  interval_bytes: bytes of each interval
        scan_len, n_intervals, n_units;  sos_offset, data_offset: where the SOS marker / the data start in the file
    """
    lay = layout or Layout()
    hy, vy = LUMA_HV[sampling]
    nY = hy * vy
    nmcu = -(-width // (8 * hy)) * -(-height // (8 * vy))
    coefs = [np.asarray(c, np.int64) for c in coefs]
    for c, per in zip(coefs, (nY, 1, 1)):
        if c.shape != (nmcu * per, 64):
            raise ValueError(f"component has {c.shape} coefficients, the frame needs {(nmcu * per, 64)}")
    qt = {}
    for i, t in zip(lay.qt_ids, qtables):
        t = [int(x) for x in t]
        if qt.setdefault(i, t) != t:
            raise ValueError(f"components share qt id {i} but not the table")
    out = bytearray(b"\xff\xd8")
    ids = _prologue(out, lay, 0xC2, width, height, hy, vy, qt)
    live, dri, records = {}, 0, []
    for sc in script:
        comps = tuple(sc.comps)
        if not comps or list(comps) != sorted(set(comps)) or not all(0 <= c <= 2 for c in comps):
            raise ValueError("a scan names one to three frame components in frame order")
        if sc.ss and len(comps) != 1:
            raise ValueError("an AC scan names one component")
        coder = _ScanCoder(sc, width, height, sampling, coefs)
        kind = ("dc_" if sc.ss == 0 else "ac_") + ("refine" if sc.ah else "first")
        keys = sorted(set(t[1] for t in coder.tok if t[0] == "s"))
        if kind == "dc_first":
            given = dict(zip((coder.keys[c] for c in comps), sc.tables)) if sc.tables is not None else {}
            keys = sorted(set(coder.keys.values()))
        elif sc.ss:
            given = {coder.key: sc.tables} if sc.tables is not None else {}
            keys = [coder.key]
        else:
            given = {}
        tables = {}
        for key in keys:
            t = given.get(key)
            if t is None:
                t = table_from_frequencies(Counter(tok[2] for tok in coder.tok if tok[0] == "s" and tok[1] == key))
            check_table(t)
            tables[key] = (list(t[0]), bytes(t[1]))
        defined = [key for key in keys if live.get(key) != tables[key]]
        _tables(out, lay, "DHT", 0xC4, [(key, tables[key]) for key in defined], _dht_payload, lay.dht_merged, _decoy_dht)
        live.update(tables)
        if sc.restart != dri or (lay.write_dri and not records):
            if not 0 <= sc.restart <= 65535:
                raise ValueError("restart interval does not fit the DRI segment")
            _segment(out, lay, "DRI", 0xDD, bytes([sc.restart >> 8, sc.restart & 255]))
            dri = sc.restart
        codes = {key: table_codes(t) for key, t in tables.items()}
        rec = dict(kind=kind, comps=comps, ss=sc.ss, se=sc.se, ah=sc.ah, al=sc.al, restart=sc.restart, tables=tables,
                   defined=defined, lengths={k: Counter() for k in keys}, symbols={k: Counter() for k in keys},
                   eob_runs=coder.eob_runs, zrl=coder.zrl, max_correction_bits=0, ff00=[], rst=[], interval_bytes=[],
                   n_units=coder.n_units)
        scan, bw, n_int = bytearray(), _Bits(), 0

        def close():
            bw.flush(lay.pad_ones)
            rec["ff00"] += [len(scan) + i for i, x in enumerate(bw.out) if x == 0xFF]
            rec["interval_bytes"].append(len(bw.out))
            scan.extend(bw.out)

        for tok in coder.tok:
            if tok[0] == "s":
                if tok[2] not in codes[tok[1]]:
                    raise ValueError(f"table {tok[1]} has no code for symbol {tok[2]:#04x}")
                code, length = codes[tok[1]][tok[2]]
                bw.put(code, length)
                rec["lengths"][tok[1]][length] += 1
                rec["symbols"][tok[1]][tok[2]] += 1
            elif tok[0] == "b":
                bw.put(tok[1], tok[2])
            elif tok[0] == "c":
                rec["max_correction_bits"] = max(rec["max_correction_bits"], len(tok[1]))
                for bit in tok[1]:
                    bw.put(bit, 1)
            else:
                close()
                scan += b"\xff" * lay.fill.get("RST", 0)
                rec["rst"].append(len(scan))
                scan += bytes([0xFF, 0xD0 + n_int % 8])
                n_int += 1
                bw = _Bits()
        close()
        rec["scan_len"], rec["n_intervals"] = len(scan), n_int + 1
        sos = bytes([len(comps)])
        for c in comps:
            td = coder.keys[c][1] if sc.ss == 0 else 0
            sos += bytes([ids[c], (td << 4) | (coder.key[1] if sc.ss else 0)])
        rec["sos_offset"] = len(out) + lay.fill.get("SOS", 0)
        _segment(out, lay, "SOS", 0xDA, sos + bytes([sc.ss, sc.se, (sc.ah << 4) | sc.al]))
        rec["data_offset"] = len(out)
        out += scan
        records.append(rec)
    out += b"\xff" * lay.fill.get("EOI", 0) + b"\xff\xd9" + lay.trailer
    return bytes(out), records


def interleave_values(coefs, sampling):
    """The progressive writer's input as a decoder holds it at the end: int32 [all blocks, 64], MCU by MCU (luma blocks,
    Cb, Cr), natural order inside a block, DC as its value."""
    nY = LUMA_BLOCKS[sampling]
    coefs = [np.asarray(c, np.int64) for c in coefs]
    nmcu = len(coefs[1])
    zz = np.concatenate([coefs[0].reshape(nmcu, nY, 64), coefs[1][:, None], coefs[2][:, None]], axis=1).reshape(-1, 64)
    out = np.zeros_like(zz)
    out[:, NATURAL_ORDER] = zz
    return out.astype(np.int32)


def standard_script(restart=0):
    """The ten scans of libjpeg's jpeg_simple_progression for three YCbCr components."""
    S = Scan
    return [S((0, 1, 2), 0, 0, 0, 1, restart), S((0,), 1, 5, 0, 2, restart), S((2,), 1, 63, 0, 1, restart),
            S((1,), 1, 63, 0, 1, restart), S((0,), 6, 63, 0, 2, restart), S((0,), 1, 63, 2, 1, restart),
            S((0, 1, 2), 0, 0, 1, 0, restart), S((2,), 1, 63, 1, 0, restart), S((1,), 1, 63, 1, 0, restart),
            S((0,), 1, 63, 1, 0, restart)]


# ------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------
def interleave_natural(coefs, sampling, raw_blocks=None):
    """The writer's input as the decoder sees it: int16 [all blocks, 64] in scan order (MCU by MCU: luma blocks, Cb,
    Cr), each block in natural order, DC still a difference.  Blocks given as raw symbol lists are read back with
    `symbols_block`."""
    nY = LUMA_BLOCKS[sampling]
    coefs = [np.array(c, np.int64) for c in coefs]
    for (c, b), syms in (raw_blocks or {}).items():
        coefs[c][b] = symbols_block(syms)
    nmcu = len(coefs[1])
    zz = np.concatenate([coefs[0].reshape(nmcu, nY, 64), coefs[1][:, None], coefs[2][:, None]], axis=1).reshape(-1, 64)
    out = np.zeros_like(zz)
    out[:, NATURAL_ORDER] = zz
    return out.astype(np.int16)


def to_differences(coefs, sampling, restart=0):
    """Blocks whose entry 0 is the DC value → the same blocks with the DC difference the scan codes (the predictor is
    the component's previous block in scan order and starts at 0 in every restart interval)."""
    out = []
    for c, blocks in enumerate(coefs):
        per = LUMA_BLOCKS[sampling] if c == 0 else 1
        b = np.array(blocks, np.int64)
        dc = b[:, 0].copy()
        prev = np.concatenate([[0], dc[:-1]])
        if restart > 0:
            prev[::restart * per] = 0
        b[:, 0] = dc - prev
        out.append(b)
    return out


def _dct_matrix():
    k, n = np.mgrid[0:8, 0:8].astype(np.float64)
    m = np.cos((2 * n + 1) * k * np.pi / 16) / 2
    m[0] /= np.sqrt(2)
    return m


def coefficients_from_pixels(img, sampling, qtables, restart=0):
    """uint8 [H, W, 3] RGB → the writer's `coefs` for a plausible picture of it: JFIF YCbCr, box-filtered chroma, edge
    replication up to whole MCUs, a float DCT and rounding.  No claim to match any encoder."""
    img = np.asarray(img, np.float64)
    h, w = img.shape[:2]
    hy, vy = LUMA_HV[sampling]
    mx, my = -(-w // (8 * hy)), -(-h // (8 * vy))
    img = np.pad(img, ((0, my * 8 * vy - h), (0, mx * 8 * hy - w), (0, 0)), mode="edge")
    r, g, b = img[..., 0], img[..., 1], img[..., 2]
    planes = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b,
              128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    for c in (1, 2):
        p = planes[c]
        planes[c] = p.reshape(my * 8, vy, mx * 8, hy).mean(axis=(1, 3))
    d = _dct_matrix()
    out = []
    for c, p in enumerate(planes):
        bh, bw = (vy, hy) if c == 0 else (1, 1)
        # [my, bh, 8, mx, bw, 8] → MCU order, then the MCU's own blocks row-major
        blk = (p - 128).reshape(my, bh, 8, mx, bw, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1, 8, 8)
        f = d @ blk @ d.T
        q = np.rint(f / np.asarray(qtables[c], np.float64).reshape(8, 8)).astype(np.int64).reshape(-1, 64)
        out.append(q[:, NATURAL_ORDER])
    return to_differences(out, sampling, restart)
