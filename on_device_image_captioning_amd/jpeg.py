"""Host side of the device JPEG decoder: a marker parser that sorts every input into
`device` / `black` / `host` and packs the header records that csrc/jpeg_decode.hip reads.

One marker walker (`_Walker`) reads every file: fill bytes, segment lengths, DQT / DHT / DRI, the SOF and the
JFIF / Adobe latches, up to each SOS.  One frame rule set (`_frame`) decides what the SOF admits.  `parse` drives
the walker to the first SOS; `parse_progressive` drives it through the whole scan script to EOI.  Neither scans
the entropy-coded data of a baseline file: finding restart markers and removing 0xFF00 stuffing is device work.

The rule behind the three kinds is that a device decode must reproduce `np.asarray(PIL.Image.open(f))` (Pillow
with libjpeg-turbo: ISLOW IDCT, fancy upsampling, table-driven YCbCr→RGB) bit for bit, and that anything the
parser does not fully understand goes to PIL, which then raises or decodes exactly as the host path does:

    device  8-bit SOF0/SOF1 Huffman, one interleaved scan of 3 YCbCr components (JFIF, Adobe transform 1,
            or component ids 1/2/3 — libjpeg's colour-space rules), luma sampling 1x1 / 2x1 / 2x2 with
            1x1 chroma, DRI present or absent
    black   1- or 4-component JPEGs (PIL mode L / CMYK): the host path never decodes them, it substitutes
            an all-black RGB canvas of the same size
    host    everything else (progressive, arithmetic, 12-bit, lossless, Adobe RGB, multi-scan, DNL,
            non-JPEG data, malformed or truncated headers, more than MAX_SCAN_BYTES after SOS)

That is the default, non_rgb="black".  Under non_rgb="convert" every file is to equal
`np.asarray(PIL.Image.open(f).convert("RGB"))` and nothing is `black`: a one-component frame (baseline here, SOF2 in
`parse_progressive`) is a `device` kind with sampling GRAY — one 8x8 block per MCU in block-raster order, whatever
sampling factors and component id the SOF declares, which libjpeg ignores for a single component — and a four-component
frame is `host`, where PIL converts it — unless the caller also passes cmyk="device": then a baseline four-component frame
(CMYK, or YCCK by Adobe transform 2) that `_frame4` admits is a `device` kind with ncomp 4, the sampling of every
component in comp_hv and the `ycck` flag; odic_jpeg_any_decode reads its records (`HEADER_ANY_DTYPE`).  To `parse`
progressive four-component files stay `host` (`PROG_CMYK_REASON`); under a draft request `plan_routes` withholds the
keyword unless draft_layouts="all", which decodes them at the draft scale (`scaled_components`).

Under layouts="all" (`parse` only; the default "common" is everything above) a baseline three-component frame that the
rules above turn away for its sampling or its colour space is a `device` kind too where `_frame3_any` admits it: every
component at its own (h, v) in 1..4 with integral ratios to the largest and at most MAX_MCU_BLOCKS blocks per MCU —
4:4:0, 4:1:1, 4:1:0, chroma sub-sampled one way under a 2x2 luma, a component 0 that is not the largest — stored as
YCbCr or as RGB (Adobe transform 0, or ids R, G, B with neither marker).  The header has `layout` set, comp_hv, the
`rgb` flag and MCU counts from the largest factors; the same call reads its records, of the same dtype.  What
still goes to the host after that:

    host    fractional sampling ratios; more than 10 blocks per MCU; progressive files (`PROG_LAYOUT_REASON`), and draft
            requests unless draft_layouts="all", with these layouts; non-interleaved multi-scan baseline files; arithmetic coding; 12-bit; three
            components with an Adobe transform other than 0 and 1, or with duplicate ids

`parse` keeps that sorting.  For the files it turns away with reason "SOF2", `parse_progressive` (below) reads the whole
scan script, locating every scan's end in the file, and packs the records odic_jpeg_decode_progressive reads.  Given
the same cmyk="device" / layouts="all" it also admits the SOF2 frames `parse` turned away with the two reasons named
above — four components, or three at a layout of `_frame3_any` — under the same frame rules and the same scan-script
rules; odic_jpeg_decode_progressive_any reads their records (`PROG_HEADER_ANY_DTYPE`).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

DEVICE, BLACK, HOST = "device", "black", "host"

#: zig-zag index → natural (row-major) index
NATURAL_ORDER = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
    54, 47, 55, 62, 63], dtype=np.int32)

MAX_SCAN_BYTES = 1 << 27           # kMaxScanBytes of csrc/jpeg_decode.hip: bit positions stay int32
LUT_BITS = 9                       # codes up to this length decode with one table lookup on the device
SAMPLING = {(1, 1): 0, (2, 1): 1, (2, 2): 2}          # luma (h, v) → 0: 4:4:4, 1: 4:2:2 (h2v1), 2: 4:2:0 (h2v2)
GRAY = 3                                              # `sampling` of a one-component frame: one 8x8 block per MCU
BLOCKS_PER_MCU = (3, 4, 6, 1)
NON_RGB = ("black", "convert")                        # what a file that is not three-component RGB / YCbCr becomes


def check_non_rgb(non_rgb):
    if non_rgb not in NON_RGB:
        raise ValueError(f"non_rgb must be 'black' or 'convert', not {non_rgb!r}")
    return non_rgb


CMYK = ("host", "device")                             # who decodes a four-component JPEG under non_rgb="convert"
MAX_MCU_BLOCKS = 10                                   # libjpeg's D_MAX_BLOCKS_IN_MCU


def check_cmyk(cmyk, non_rgb):
    if cmyk not in CMYK:
        raise ValueError(f"cmyk must be 'host' or 'device', not {cmyk!r}")
    if cmyk == "device" and non_rgb != "convert":
        raise ValueError("cmyk='device' decodes four-component files to their RGB conversion: it needs "
                         "non_rgb='convert' (under non_rgb='black' they are black canvases)")
    return cmyk



LAYOUTS = ("common", "all")                           # which three-component baseline layouts are a device kind


def check_layouts(layouts):
    if layouts not in LAYOUTS:
        raise ValueError(f"layouts must be 'common' or 'all', not {layouts!r}")
    return layouts


DRAFT_LAYOUTS = ("common", "all")                     # which layouts a draft request leaves to the device
                                                      # ("all": also the kinds of cmyk="device" / layouts="all")


def check_draft_layouts(draft_layouts):
    if draft_layouts not in DRAFT_LAYOUTS:
        raise ValueError(f"draft_layouts must be 'common' or 'all', not {draft_layouts!r}")
    return draft_layouts


# odic_jpeg_header (include/odic_hip.h), field for field
HEADER_DTYPE = np.dtype([
    ("data_off", "<i8"), ("data_end", "<i8"), ("out_off", "<i8"), ("scan_off", "<i8"), ("coef_off", "<i8"),
    ("plane_off", "<i8"),
    ("int_off", "<i4"), ("unit_off", "<i4"), ("width", "<i4"), ("height", "<i4"), ("sampling", "<i4"),
    ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("restart", "<i4"), ("n_intervals", "<i4"), ("n_units", "<i4"),
    ("qt", "<u2", (3, 64)), ("lut", "<u2", (6, 512)), ("maxcode", "<i4", (6, 18)), ("valoff", "<i4", (6, 18)),
    ("huffval", "u1", (6, 256)),
], align=True)
# odic_jpeg_header_any (include/odic_hip.h), field for field: three or four components, each with its own sampling;
# `color` as in PROG_HEADER_ANY_DTYPE (three components: stored as RGB; four: YCCK)
HEADER_ANY_DTYPE = np.dtype([
    ("data_off", "<i8"), ("data_end", "<i8"), ("out_off", "<i8"), ("scan_off", "<i8"), ("coef_off", "<i8"),
    ("plane_off", "<i8"),
    ("int_off", "<i4"), ("unit_off", "<i4"), ("width", "<i4"), ("height", "<i4"), ("color", "<i4"),
    ("mcus_x", "<i4"), ("mcus_y", "<i4"), ("restart", "<i4"), ("n_intervals", "<i4"), ("n_units", "<i4"),
    ("h", "<i4", (4,)), ("v", "<i4", (4,)), ("ncomp", "<i4"), ("pad", "<i4"),
    ("qt", "<u2", (4, 64)), ("lut", "<u2", (8, 512)), ("maxcode", "<i4", (8, 18)), ("valoff", "<i4", (8, 18)),
    ("huffval", "u1", (8, 256)),
], align=True)


@dataclass
class HuffTable:
    bits: list            # number of codes of each length 1..16
    vals: bytes           # symbols in code order


@dataclass
class JpegHeader:
    kind: str
    width: int = 0
    height: int = 0
    ncomp: int = 0
    sampling: int = -1                                   # index into SAMPLING values (device kind only)
    comp_ids: list = field(default_factory=list)
    comp_hv: list = field(default_factory=list)          # [(h, v)] per frame component
    qtables: list = field(default_factory=list)          # per component: int32[64] natural order
    dc_tables: list = field(default_factory=list)        # per component HuffTable
    ac_tables: list = field(default_factory=list)
    restart_interval: int = 0                            # DRI value (0: none)
    data_offset: int = 0                                 # first byte of the entropy-coded data
    reason: str = ""
    ycck: bool = False                                   # four components: Adobe transform 2 (YCCK), else CMYK as stored
    layout: bool = False                                 # three components admitted by `_frame3_any` (layouts="all")
    rgb: bool = False                                    # ... stored as RGB (no colour conversion), else YCbCr
    app1: list = field(default=None, compare=False, repr=False)     # APP1 payloads ahead of the first SOS, where the
                                                                     # walk got that far (`header_orientation`)

    @property
    def mcus_x(self):                                    # the MCU spans the largest factors: component 0's in every
        return -(-self.width // (8 * max(h for h, _ in self.comp_hv)))      # frame but a `layout` one

    @property
    def mcus_y(self):
        return -(-self.height // (8 * max(v for _, v in self.comp_hv)))


class _Bad(Exception):
    pass


def _u16(b, i):
    if i + 2 > len(b):
        raise _Bad("truncated")
    return (b[i] << 8) | b[i + 1]


def parse(blob, non_rgb: str = "black", cmyk: str = "host", layouts: str = "common") -> JpegHeader:
    """Walk the markers of one file up to SOS → JpegHeader with its kind; never raises on a file's content.
    non_rgb="convert": a one-component frame is a device kind (sampling GRAY) and a four-component one goes to the
    host, where PIL converts it; the default "black" sorts both as BLACK.
    cmyk="device" (with non_rgb="convert" only): a baseline four-component frame that `_frame4` admits is a device
    kind with ncomp 4, comp_hv and `ycck`; progressive four-component files stay HOST, with a reason of their own.
    A caller with a draft request leaves cmyk at "host" unless it decodes these files at the draft scale
    (`plan_routes` with draft_layouts="all").
    layouts="all": a baseline three-component frame that the common rules turn away for its sampling or colour space
    and `_frame3_any` admits is a device kind with `layout` set, comp_hv and `rgb`; progressive ones stay HOST, with a
    reason of their own.  A file the common rules admit parses as it does without the keyword.  A caller with a draft
    request leaves layouts at "common" likewise, unless draft_layouts="all"."""
    check_non_rgb(non_rgb)
    check_cmyk(cmyk, non_rgb)
    check_layouts(layouts)
    try:
        return _parse(memoryview(blob).cast("B") if not isinstance(blob, bytes) else blob, non_rgb, cmyk, layouts)
    except _Bad as e:
        return JpegHeader(HOST, reason=str(e))
    except (IndexError, ValueError) as e:
        return JpegHeader(HOST, reason=f"malformed: {e}")


def _read_dqt(s, qt):
    """One DQT segment → qt[id] = int32[64] in natural order."""
    j = 0
    while j < len(s):
        pq, tq = s[j] >> 4, s[j] & 15
        if pq > 1 or tq > 3:
            raise _Bad("bad DQT")
        size = 64 * (pq + 1)
        if j + 1 + size > len(s):
            raise _Bad("bad DQT length")
        raw = np.frombuffer(s, dtype=">u2" if pq else "u1", count=64, offset=j + 1).astype(np.int32)
        nat = np.zeros(64, np.int32)
        nat[NATURAL_ORDER] = raw
        qt[tq] = nat
        j += 1 + size


def _read_dht(s, dht):
    """One DHT segment → dht[(class, id)] = HuffTable."""
    j = 0
    while j < len(s):
        tc, th = s[j] >> 4, s[j] & 15
        if tc > 1 or th > 3 or j + 17 > len(s):
            raise _Bad("bad DHT")
        bits = list(s[j + 1:j + 17])
        cnt = sum(bits)
        if cnt > 256 or j + 17 + cnt > len(s):
            raise _Bad("bad DHT length")
        vals = s[j + 17:j + 17 + cnt]
        code = 0
        for length in range(1, 17):                   # libjpeg jpeg_make_d_derived_tbl checks
            code += bits[length - 1]
            if code >= (1 << length):
                raise _Bad("bad Huffman table")
            code <<= 1
        if tc == 0 and any(v > 15 for v in vals):
            raise _Bad("bad DC symbol")
        dht[(tc, th)] = HuffTable(bits, vals)
        j += 17 + cnt


class _Walker:
    """The marker walk behind both parsers (libjpeg's jdmarker.c rules): what the segments ahead of a scan define."""

    def __init__(self, b):
        if len(b) < 4 or b[0] != 0xFF or b[1] != 0xD8:
            raise _Bad("not a JPEG")
        self.b, self.i = b, 2                         # i: where the walk goes on after an SOS; the caller moves it past
                                                      # the scan's data
        self.qt, self.dht = {}, {}                    # id → int32[64]; (class, id) → HuffTable
        self.dri, self.sof = 0, None                  # sof: (marker, precision, height, width, nc, [(id, h, v, tq)])
        self.jfif = self.adobe = False
        self.adobe_transform = None
        self.app1 = []                                # payload of every APP1 ahead of the first SOS (`exif_orientation`)

    def scans(self, script):
        """Generator of the payload of every SOS segment, self.i behind it.  script=False (`parse`): the caller
        stops at the first SOS.  script=True (`parse_progressive`): the caller sets self.i to the end of the scan's
        data and goes on; the walk ends at EOI."""
        b, n, i = self.b, len(self.b), self.i
        before = True                                 # no SOS yet
        while True:
            if i + 2 > n:
                raise _Bad("truncated")
            if b[i] != 0xFF:
                raise _Bad("junk between markers")
            m = b[i + 1]
            if m == 0xFF:                             # fill byte
                i += 1
                continue
            if m == 0xD9 and script:                  # a scan script ends at EOI, and says so when it comes too early;
                if before:                            # to `parse` an EOI is one more unexpected marker, below
                    raise _Bad("EOI before SOS")
                return
            if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7 or m == 0xD9:      # SOI, TEM, RSTn: no segment, and no place here
                raise _Bad(f"unexpected marker {m:02X} before SOS" if before else f"unexpected marker {m:02X}")
            seg_len = _u16(b, i + 2)
            if seg_len < 2 or i + 2 + seg_len > n:
                raise _Bad("truncated segment")
            s = bytes(b[i + 4:i + 2 + seg_len])
            i += 2 + seg_len
            if m == 0xC4:
                _read_dht(s, self.dht)
            elif m == 0xDD:
                if len(s) != 2:
                    raise _Bad("bad DRI")
                self.dri = (s[0] << 8) | s[1]
            elif 0xE0 <= m <= 0xEF or m == 0xFE:      # APPn / COM: skipped, but for libjpeg's two colour-space latches
                                                      # and the APP1 payloads, kept for `exif_orientation`
                if before and m == 0xE0 and len(s) >= 14 and s[:5] == b"JFIF\x00":        # APP0_DATA_LEN
                    self.jfif = True
                elif before and m == 0xEE and len(s) >= 12 and s[:5] == b"Adobe":         # APP14_DATA_LEN
                    self.adobe, self.adobe_transform = True, s[11]
                elif before and m == 0xE1:
                    self.app1.append(s)
            elif m == 0xDA:
                before, self.i = False, i
                yield s
                i = self.i
            elif not before:                          # between scans only DHT, DRI, APPn / COM and SOS
                raise _Bad(f"marker {m:02X} between scans")      # DQT (latched per component by libjpeg), DNL, ...
            elif m == 0xDB:
                _read_dqt(s, self.qt)
            elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):    # every SOF; C4 is DHT, above
                if self.sof is not None:
                    raise _Bad("second SOF")
                if len(s) < 6:
                    raise _Bad("short SOF")
                nc = s[5]
                if len(s) != 6 + 3 * nc:
                    raise _Bad("bad SOF length")
                self.sof = (m, s[0], _u16(s, 1), _u16(s, 3), nc,
                            [(s[6 + 3 * k], s[7 + 3 * k] >> 4, s[7 + 3 * k] & 15, s[8 + 3 * k]) for k in range(nc)])
            else:
                raise _Bad(f"marker {m:02X}")


PROG_CMYK_REASON = "4 components, progressive (SOF2)"
PROG_LAYOUT_REASON = "3 components, progressive (SOF2), outside the common layouts"


def _frame4(w, header, sof_kinds=(0xC0, 0xC1)):
    """The four-component half of `_frame` for cmyk="device", by libjpeg's rules (jdapimin.c default_decompress_parms,
    jdinput.c): the colour space comes from the Adobe marker alone — transform 2 is YCCK, transform 0 and no Adobe
    marker (a JFIF marker does not matter) are CMYK; any other transform makes libjpeg warn and guess, which is the
    host's.  Component 0 carries the MCU's size; every other component is 1x1 or shares it.  sof_kinds: the frame
    markers of the parser that asks; the other parser's get that parser's reason."""
    m, _, height, width, _, comps = w.sof
    if m not in sof_kinds:
        raise _Bad(PROG_CMYK_REASON if m == 0xC2 else f"SOF{m - 0xC0}")
    if width == 0 or height == 0:
        raise _Bad("DNL / empty frame")
    t = w.adobe_transform if w.adobe else 0
    if t not in (0, 2):
        raise _Bad(f"4 components with Adobe transform {t}")
    ids = [c[0] for c in comps]
    if len(set(ids)) != 4:
        raise _Bad("duplicate component ids")
    hv = [(c[1], c[2]) for c in comps]
    if hv[0] not in SAMPLING or any(x != (1, 1) and x != hv[0] for x in hv[1:]):
        raise _Bad(f"sampling {hv}")
    blocks = sum(h * v for h, v in hv)
    if blocks > MAX_MCU_BLOCKS:
        raise _Bad(f"{blocks} blocks per MCU")
    for c in comps:
        if c[3] not in w.qt:
            raise _Bad("missing DQT")
    return header(DEVICE, width=width, height=height, ncomp=4, comp_ids=ids, comp_hv=hv,
                  qtables=[w.qt[c[3]] for c in comps], ycck=t == 2)


def _frame3_any(w, header, sof_kinds=(0xC0, 0xC1)):
    """The three-component frames of layouts="all" that the common rules turn away, by libjpeg's rules.
    jdapimin.c default_decompress_parms: a JFIF marker means YCbCr; else Adobe transform 0 is RGB and 1 is YCbCr (any
    other makes libjpeg warn and guess: the host's); with neither marker ids 1, 2, 3 are YCbCr, R, G, B are RGB and
    anything else is taken for YCbCr.  jdinput.c initial_setup / per_scan_setup: factors in 1..4, at most
    MAX_MCU_BLOCKS blocks per MCU, the MCU spans the largest factors.  jdsample.c jinit_upsampler: the ratio of the
    largest factor to each component's has to be integral ("fractional sampling not implemented")."""
    m, _, height, width, _, comps = w.sof
    hv = [(c[1], c[2]) for c in comps]
    if m not in sof_kinds:
        raise _Bad(f"{PROG_LAYOUT_REASON}: {hv}" if m == 0xC2 else f"SOF{m - 0xC0}")
    if width == 0 or height == 0:
        raise _Bad("DNL / empty frame")
    ids = [c[0] for c in comps]
    if w.jfif:
        rgb = False
    elif w.adobe:
        if w.adobe_transform not in (0, 1):
            raise _Bad(f"3 components with Adobe transform {w.adobe_transform}")
        rgb = w.adobe_transform == 0
    else:
        rgb = ids == [0x52, 0x47, 0x42]
    if len(set(ids)) != 3:
        raise _Bad("duplicate component ids")
    if any(not (1 <= h <= 4 and 1 <= v <= 4) for h, v in hv):
        raise _Bad(f"sampling {hv}")
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    if any(hmax % h or vmax % v for h, v in hv):
        raise _Bad(f"fractional sampling {hv}")
    blocks = sum(h * v for h, v in hv)
    if blocks > MAX_MCU_BLOCKS:
        raise _Bad(f"{blocks} blocks per MCU")
    for c in comps:
        if c[3] not in w.qt:
            raise _Bad("missing DQT")
    return header(DEVICE, width=width, height=height, ncomp=3, comp_ids=ids, comp_hv=hv,
                  qtables=[w.qt[c[3]] for c in comps], layout=True, rgb=rgb)


def _common3(w):
    """Whether the common rules of `_frame` admit this three-component frame's colour space and sampling."""
    comps = w.sof[5]
    ycc = w.jfif or (w.adobe_transform == 1 if w.adobe else [c[0] for c in comps] == [1, 2, 3])
    hv = [(c[1], c[2]) for c in comps]
    return ycc and hv[1] == (1, 1) and hv[2] == (1, 1) and hv[0] in SAMPLING


def _frame(w, header, sof_kinds, distinct_ids, non_rgb="black", cmyk="host", layouts="common"):
    """What the frame admits, by libjpeg's rules, at the first SOS → header(BLACK) or header(DEVICE) with the frame
    fields; anything else raises.  sof_kinds: {C0, C1} for `parse`, {C2} for `parse_progressive`."""
    if w.sof is None:
        raise _Bad("SOS before SOF")
    m, prec, height, width, nc, comps = w.sof
    if prec != 8:
        raise _Bad(f"{prec}-bit")
    if nc not in (1, 3, 4):
        raise _Bad(f"{nc} components")
    if nc in (1, 4) and m in (0xC0, 0xC1, 0xC2) and non_rgb == "black":
        # PIL opens these as mode L / CMYK and the host path substitutes a black RGB canvas without decoding
        if width == 0 or height == 0:
            raise _Bad("empty frame")
        return header(BLACK, width=width, height=height, ncomp=nc)
    if nc == 4 and m in (0xC0, 0xC1, 0xC2):           # non_rgb="convert": Adobe inversion, YCCK and PIL's CMYK → RGB are
        if cmyk == "device":                          # the host's, whichever parser asks, unless `parse` was told
            return _frame4(w, header, sof_kinds)      # cmyk="device"
        raise _Bad("4 components (CMYK / YCCK)")
    if layouts == "all" and nc == 3 and m in (0xC0, 0xC1, 0xC2) and not _common3(w):
        return _frame3_any(w, header, sof_kinds)
    if m not in sof_kinds:
        raise _Bad(f"SOF{m - 0xC0}")
    if width == 0 or height == 0:
        raise _Bad("DNL / empty frame")
    if nc == 1:
        # libjpeg decodes a one-component frame as one block per MCU in block-raster order whatever sampling factors
        # and component id the SOF declares, and no colour-space latch applies: the header says (1, 1) for all of them
        if comps[0][3] not in w.qt:
            raise _Bad("missing DQT")
        return header(DEVICE, width=width, height=height, ncomp=1, sampling=GRAY, comp_ids=[comps[0][0]],
                      comp_hv=[(1, 1)], qtables=[w.qt[comps[0][3]]])
    ids = [c[0] for c in comps]
    if w.jfif:
        ycc = True
    elif w.adobe:
        ycc = w.adobe_transform == 1
    else:
        ycc = ids == [1, 2, 3]
    if not ycc:
        raise _Bad("not YCbCr")
    if distinct_ids and len(set(ids)) != 3:           # progressive only: its scans name components by id
        raise _Bad("duplicate component ids")
    hv = [(c[1], c[2]) for c in comps]
    if hv[1] != (1, 1) or hv[2] != (1, 1) or hv[0] not in SAMPLING:
        raise _Bad(f"sampling {hv}")
    for c in comps:
        if c[3] not in w.qt:
            raise _Bad("missing DQT")
    return header(DEVICE, width=width, height=height, ncomp=3, sampling=SAMPLING[hv[0]], comp_ids=ids, comp_hv=hv,
                  qtables=[w.qt[c[3]] for c in comps])


def _parse(b, non_rgb="black", cmyk="host", layouts="common") -> JpegHeader:
    w = _Walker(b)
    s = next(w.scans(script=False))                   # the first SOS; whatever keeps the walk from it raises
    hd = _frame(w, JpegHeader, (0xC0, 0xC1), distinct_ids=False, non_rgb=non_rgb, cmyk=cmyk, layouts=layouts)
    hd.app1 = w.app1
    if hd.kind != DEVICE:
        return hd
    # SOS: one baseline scan of all the frame's components (three or four interleaved, or the one of a gray frame), in
    # frame order
    ns = s[0] if len(s) >= 1 else 0
    if ns != hd.ncomp or len(s) != 1 + 2 * ns + 3:
        raise _Bad("not one interleaved scan")
    sel = [(s[1 + 2 * k], s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(ns)]
    if [x[0] for x in sel] != hd.comp_ids:
        raise _Bad("scan component order")
    ss, se, ah_al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]
    if ss != 0 or se != 63 or ah_al != 0:
        raise _Bad("bad spectral selection")
    for _, td, ta in sel:
        if (0, td) not in w.dht or (1, ta) not in w.dht:
            raise _Bad("missing DHT")                   # libjpeg-turbo would substitute the standard tables
        hd.dc_tables.append(w.dht[(0, td)])
        hd.ac_tables.append(w.dht[(1, ta)])
    if w.i >= len(b):
        raise _Bad("no scan data")
    if len(b) - w.i > MAX_SCAN_BYTES:
        raise _Bad("scan longer than the device decoder's bit positions allow")
    hd.restart_interval, hd.data_offset = w.dri, w.i
    return hd


# ---------------------------------------------------------------------------------------------------------------
# EXIF orientation (tag 0x0112): what `ImageOps.exif_transpose` would do to the file.  The rule of this file applies:
# own code reads the plain form only — exactly one `Exif\0\0` APP1 ahead of the first SOS, a TIFF header `II` / `MM`
# with magic 42, IFD0 walked to its end, one entry 0x0112 of type SHORT or LONG with count 1 — and everything else
# (several Exif APP1s, which Pillow concatenates; another entry type or count; an Exif block that cannot be walked; no
# Orientation in Exif but an XMP packet that names tiff:Orientation; a file the walker turns away) is Pillow's to
# decide: `Image.open(...).getexif().get(0x0112)` reads headers and decodes no pixels.  Asking Pillow changes where the
# number comes from, never the decode route.
# ---------------------------------------------------------------------------------------------------------------
ORIENTATIONS = ("ignore", "exif")
_EXIF, _XMP = b"Exif\x00\x00", b"http://ns.adobe.com/xap/1.0/\x00"
#: orientation → (mirror x, mirror y, swap the axes): source pixel (y, x) of an H x W image lands at (u, v) with
#: u = H-1-y if mirror y else y and v = W-1-x if mirror x else x, or at (v, u) when the axes swap (csrc/orient.hip)
ORIENT_OPS = {1: (False, False, False), 2: (True, False, False), 3: (True, True, False), 4: (False, True, False),
              5: (False, False, True), 6: (False, True, True), 7: (True, True, True), 8: (True, False, True)}


def check_orientation(orientation):
    if orientation not in ORIENTATIONS:
        raise ValueError(f"orientation must be 'ignore' or 'exif', not {orientation!r}")
    return orientation


def transpose_method(orientation: int):
    """The `Image.Transpose` method `ImageOps.exif_transpose` applies for an orientation 2..8."""
    from PIL import Image
    t = Image.Transpose
    return {2: t.FLIP_LEFT_RIGHT, 3: t.ROTATE_180, 4: t.FLIP_TOP_BOTTOM, 5: t.TRANSPOSE, 6: t.ROTATE_270,
            7: t.TRANSVERSE, 8: t.ROTATE_90}[orientation]


def effective_orientation(tag) -> int:
    """Pillow's tag value → the orientation `exif_transpose` acts on: an int 2..8, else 1 (absent, 0, 9, the ASCII
    "6" and the BYTE b"\x06" that Pillow reports but does not transpose by)."""
    return tag if isinstance(tag, int) and not isinstance(tag, bool) and 2 <= tag <= 8 else 1


def pil_orientation(im) -> int:
    """The effective orientation of an opened PIL image, any format."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return effective_orientation(im.getexif().get(0x0112))


def _plain_orientation(app1):
    """The APP1 payloads ahead of the first SOS → the raw tag value of the plain form (1: no tag anywhere), or None:
    ask Pillow."""
    import struct
    exif = [s for s in app1 if s.startswith(_EXIF)]
    xmp = any(s.startswith(_XMP) and b"tiff:Orientation" in s for s in app1)
    if len(exif) > 1:
        return None
    if exif:
        t = exif[0][6:]
        if t[:4] == b"II\x2a\x00":
            e = "<"
        elif t[:4] == b"MM\x00\x2a":
            e = ">"
        else:
            return None
        if len(t) < 8:
            return None
        off = struct.unpack_from(e + "I", t, 4)[0]
        if off + 2 > len(t):
            return None
        n = struct.unpack_from(e + "H", t, off)[0]
        if off + 2 + 12 * n + 4 > len(t):             # the entries and the offset of the next IFD behind them
            return None
        found = []
        for k in range(n):
            tag, typ, cnt = struct.unpack_from(e + "HHI", t, off + 2 + 12 * k)
            if tag == 0x0112:
                if typ not in (3, 4) or cnt != 1:
                    return None
                found.append(struct.unpack_from(e + ("H" if typ == 3 else "I"), t, off + 2 + 12 * k + 8)[0])
        if len(found) > 1:
            return None
        if found:
            return found[0]
    return None if xmp else 1


def exif_orientation(blob) -> int:
    """The orientation 1..8 `ImageOps.exif_transpose(Image.open(f))` acts on: 1 wherever Pillow does not transpose
    (no tag, a value outside 2..8, a tag Pillow reads as something other than an int, a file Pillow cannot open).
    Looks at the segments ahead of the first SOS only, as Pillow's `_open` does; never raises on a file's content."""
    b = blob if isinstance(blob, bytes) else bytes(blob)
    try:
        w = _Walker(b)
        next(w.scans(script=False))
        tag = _plain_orientation(w.app1)
    except (_Bad, IndexError, ValueError, StopIteration):
        tag = None
    return _pillow_orientation(b) if tag is None else effective_orientation(tag)


def _pillow_orientation(b) -> int:
    import io
    import warnings
    from PIL import Image
    try:
        with warnings.catch_warnings():                  # a corrupt Exif block: Pillow warns and reports no tag
            warnings.simplefilter("ignore")
            with Image.open(io.BytesIO(b)) as im:
                return pil_orientation(im)
    except Exception:                                    # not an image Pillow opens: the decode route says so
        return 1


def header_orientation(hd, blob) -> int:
    """`exif_orientation(blob)` for a file `parse` / `parse_progressive` has walked already: from the APP1 payloads the
    header kept, without a second walk; a header without them (the walk ended early) reads the file."""
    if hd.app1 is None:
        return exif_orientation(blob)
    tag = _plain_orientation(hd.app1)
    return _pillow_orientation(blob) if tag is None else effective_orientation(tag)


def oriented_size(size, orientation: int):
    """(width, height) of an image of `size` after the orientation is applied."""
    return (size[1], size[0]) if ORIENT_OPS[orientation][2] else (size[0], size[1])


def orient_box(box, size, orientation: int, inverse: bool = False):
    """An (l, t, r, b) box between the stored pixel grid and the oriented one.  size: (width, height) of the image AS
    STORED, for both directions.  inverse=False: a box on the stored grid → the same pixels on the oriented grid;
    inverse=True: a box on the oriented grid (e.g. `grounding.source_box` of an image decoded with
    orientation="exif") → the box on the file as stored."""
    if orientation not in ORIENT_OPS:
        raise ValueError(f"orientation must lie in 1..8, not {orientation!r}")
    fx, fy, swap = ORIENT_OPS[orientation]
    W, H = size
    l, t, r, b = box
    if not inverse:
        v0, v1 = (W - r, W - l) if fx else (l, r)
        u0, u1 = (H - b, H - t) if fy else (t, b)
        return (u0, v0, u1, v1) if swap else (v0, u0, v1, u1)
    (u0, u1), (v0, v1) = ((l, r), (t, b)) if swap else ((t, b), (l, r))
    x0, x1 = (W - v1, W - v0) if fx else (v0, v1)
    y0, y1 = (H - u1, H - u0) if fy else (u0, u1)
    return (x0, y0, x1, y1)


@dataclass
class RoutePlan:
    """Who decodes each file of one `decode_jpeg` call (`plan_routes`)."""
    hdrs: list                     # JpegHeader / ProgHeader per file
    scales: list                   # the draft scale of each (1 without a draft request, and for a HOST kind)
    sizes: list                    # (width, height) each decodes to
    routes: list                   # "device", "device-progressive", "device-cmyk", "device-layout",
                                   # "device-progressive-cmyk", "device-progressive-layout", "host" or "black"
    base: list                     # indices of the files of each device group (GROUP_KINDS), in input order:
    prog: list                     # odic_jpeg_decode, odic_jpeg_decode_progressive,
    own: list                      # odic_jpeg_any_decode (per-component sampling: three and four components together),
    pany: list                     # odic_jpeg_decode_progressive_any

    @property
    def groups(self):
        """[(kind, file indices)] of the device groups in GROUP_KINDS order, empty ones included."""
        return [(kind, getattr(self, kind)) for kind in GROUP_KINDS]

    @property
    def order(self):
        return [i for _, idx in self.groups for i in idx]


def plan_routes(blobs, progressive="host", draft=None, non_rgb="black", cmyk="host", layouts="common",
                draft_layouts="common", max_bytes=None) -> RoutePlan:
    """Parse every file and sort it into its decode route: the host half of `DevicePreprocessor.decode_jpeg`, whose
    keywords these are.  draft: None or a positive (width, height).  Under a draft request cmyk= and layouts= are
    withheld from the parsers — their files are HOST kinds, decoded by PIL with the same request — unless
    draft_layouts="all", which passes them through: the files keep their four route names and their scale is the one
    `draft_scale` picks.  Without a draft request draft_layouts changes nothing.  max_bytes: a device kind whose
    decoded image is larger goes to PIL like a HOST kind (route "host")."""
    if progressive not in ("device", "host"):
        raise ValueError(f"progressive must be 'device' or 'host', not {progressive!r}")
    check_non_rgb(non_rgb)
    check_cmyk(cmyk, non_rgb)
    check_layouts(layouts)
    check_draft_layouts(draft_layouts)
    opt = () if non_rgb == "black" else (non_rgb,)                   # the default's calls stay as they are
    own_kinds = draft is None or draft_layouts == "all"
    copt = {"cmyk": cmyk} if cmyk != "host" and own_kinds else {}
    if layouts != "common" and own_kinds:
        copt["layouts"] = layouts
    hdrs = [parse(b, *opt, **copt) for b in blobs]
    if progressive == "device":
        for i, h in enumerate(hdrs):
            if h.kind == HOST and h.reason == "SOF2":
                ph = parse_progressive(blobs[i], *opt)
                if ph.kind == DEVICE:
                    hdrs[i] = ph
            elif h.kind == HOST and (h.reason == PROG_CMYK_REASON or h.reason.startswith(PROG_LAYOUT_REASON)):
                ph = parse_progressive(blobs[i], *opt, **copt)       # `parse` gives these reasons under copt only
                if ph.kind == DEVICE:
                    hdrs[i] = ph
    scales = [draft_scale((h.width, h.height), draft) if draft is not None and h.kind != HOST else 1 for h in hdrs]
    sizes = [scaled_size((h.width, h.height), s) for h, s in zip(hdrs, scales)]          # (width, height)
    # an oversized file goes to PIL like a host-kind one: the host path decodes it before its size check fails
    routes = ["host" if h.kind == DEVICE else h.kind for h in hdrs]          # a device kind left so is oversized
    groups = {kind: [] for kind in GROUP_KINDS}
    for i, h in enumerate(hdrs):
        if h.kind != DEVICE or (max_bytes is not None and sizes[i][0] * sizes[i][1] * 3 > max_bytes):
            continue
        prog = isinstance(h, ProgHeader)
        own = h.ncomp == 4 or h.layout                               # every component with its own sampling
        groups[("pany" if prog else "own") if own else ("prog" if prog else "base")].append(i)
        routes[i] = ("device" + ("-progressive" if prog else "")
                     + (("-cmyk" if h.ncomp == 4 else "-layout") if own else ""))
    return RoutePlan(hdrs, scales, sizes, routes, **groups)


_TABLE_CACHE: dict = {}


def device_tables(t: HuffTable):
    """One Huffman table in the device lookup form: (lut uint16[512] = (len << 8) | symbol for codes of at most
    LUT_BITS bits, 0 elsewhere; maxcode int32[18] (largest code of each length, -1 if none); valoff int32[18]
    (index into huffval minus the first code of that length); huffval uint8[256]).  Files of one encoder share
    their tables, so the expanded form is cached by content."""
    key = (bytes(t.bits), bytes(t.vals))
    hit = _TABLE_CACHE.get(key)
    if hit is None:
        if len(_TABLE_CACHE) >= 1024:
            _TABLE_CACHE.clear()
        hit = _TABLE_CACHE[key] = _expand_table(t)
    return hit


def _expand_table(t: HuffTable):
    lut = np.zeros(1 << LUT_BITS, np.uint16)
    maxcode = np.full(18, -1, np.int32)
    valoff = np.zeros(18, np.int32)
    huffval = np.zeros(256, np.uint8)
    huffval[:len(t.vals)] = np.frombuffer(bytes(t.vals), np.uint8)
    code, p = 0, 0
    for length in range(1, 17):
        cnt = t.bits[length - 1]
        if cnt:
            valoff[length] = p - code
            for c in range(code, code + cnt):
                if length <= LUT_BITS:
                    sh = LUT_BITS - length
                    lut[c << sh:(c + 1) << sh] = (length << 8) | t.vals[p + c - code]
            code += cnt
            p += cnt
            maxcode[length] = code - 1
        code <<= 1
    return lut, maxcode, valoff, huffval


def n_intervals(h: JpegHeader) -> int:
    total = h.mcus_x * h.mcus_y
    r = h.restart_interval or total
    return -(-total // r)


def draft_scale(size, requested) -> int:
    """The scale Pillow's `Image.draft(mode, requested)` picks for a JPEG of `size` (both (width, height)):
    the largest of 8, 4, 2, 1 that does not exceed min(width // req_w, height // req_h)."""
    scale = min(size[0] // requested[0], size[1] // requested[1])
    return next((s for s in (8, 4, 2) if scale >= s), 1)


def scaled_size(size, scale):
    """(width, height) a frame of `size` decodes to at 1 / scale: what `im.size` becomes after the draft."""
    return (size[0] + scale - 1) // scale, (size[1] + scale - 1) // scale


def scaled_components(comp_hv, scale):
    """libjpeg's per-component geometry of a frame decoded at 1 / scale (scale 1, 2, 4 or 8) → [(n, rh, rv)] per
    component: the side n in {1, 2, 4, 8} of the block its inverse transform produces and the integral upsampling
    factors that remain across and down.  jdmaster.c: every component starts at 8 / scale and doubles while it is below
    8 and the doubled block still divides the largest component's extent in both directions; jdsample.c then upsamples
    by (hmax · min) / (h · n) and (vmax · min) / (v · n).  4:2:0 chroma at 1/2 is transformed at 8 and not upsampled,
    4:2:2 chroma stays at 4 (h2v1), 4:1:1 chroma never doubles.  The triangle filters apply only while 8 / scale > 1."""
    if scale not in (1, 2, 4, 8):
        raise ValueError(f"scale must be 1, 2, 4 or 8, not {scale!r}")
    mn = 8 // scale
    hmax, vmax = max(h for h, _ in comp_hv), max(v for _, v in comp_hv)
    out = []
    for h, v in comp_hv:
        n = mn
        while n < 8 and (hmax * mn) % (h * n * 2) == 0 and (vmax * mn) % (v * n * 2) == 0:
            n *= 2
        out.append((n, hmax * mn // (h * n), vmax * mn // (v * n)))
    return out


def scaled_plane_bytes(h, scale=1):
    """Bytes of every component's sample plane of a per-component-sampling header decoded at 1 / scale: mcus_x · n · h
    by mcus_y · n · v samples at the component's own n (`scaled_components`), each plane rounded up to a multiple of 16
    bytes so that the next one starts where the IDCT's n-aligned row stores need it."""
    nmcu = h.mcus_x * h.mcus_y
    return [(nmcu * a * b * n * n + 15) // 16 * 16
            for (a, b), (n, _, _) in zip(h.comp_hv, scaled_components(h.comp_hv, scale))]


def _per_component(dtype) -> bool:
    """The record family of a header dtype: per-component (`h` / `v` per component, `ncomp`, `color`; planes at each
    component's own size, output offsets rounded up to whole words for the colour pass's 32-bit stores) against common
    (one `sampling` word)."""
    return "h" in dtype.names


def _place_image(r, h, tot, out_offs, out_bytes, scale=1):
    """The per-image part of both packers: geometry, quantisation tables and the output / coefficient / plane offsets
    into record r, the running totals and maxima into tot → (MCUs, output bytes after this image).  The record keeps
    the frame's own geometry, which the entropy decoders need; the output bytes and the maxima that size the colour
    launch are those of the frame decoded at 1 / scale (odic_jpeg_decode_scaled).  A record with per-component sampling
    reserves its planes at the per-component transform sizes of that scale (`scaled_plane_bytes`)."""
    if scale not in (1, 2, 4, 8):
        raise ValueError(f"scale must be 1, 2, 4 or 8, not {scale!r}")
    width, height = scaled_size((h.width, h.height), scale)
    nmcu = h.mcus_x * h.mcus_y
    own = _per_component(r.dtype)
    blocks = nmcu * (sum(a * b for a, b in h.comp_hv) if own else BLOCKS_PER_MCU[h.sampling])
    r["out_off"], r["coef_off"], r["plane_off"] = out_bytes, tot["total_blocks"], tot["total_plane_bytes"]
    r["width"], r["height"] = h.width, h.height
    if own:                                           # three or four components, told apart by ncomp
        r["ncomp"], r["color"] = h.ncomp, int(h.ycck if h.ncomp == 4 else h.rgb)
        r["h"][:h.ncomp], r["v"][:h.ncomp] = [a for a, _ in h.comp_hv], [b for _, b in h.comp_hv]
    else:
        r["sampling"] = h.sampling
    r["mcus_x"], r["mcus_y"] = h.mcus_x, h.mcus_y
    for c in range(h.ncomp):                          # a gray frame: qt[0], the rest stays zero
        r["qt"][c] = h.qtables[c]
    out_offs.append(out_bytes)
    tot["total_blocks"] += blocks
    tot["total_plane_bytes"] += sum(scaled_plane_bytes(h, scale)) if own else (blocks * 64 + 15) // 16 * 16
    tot["max_width"] = max(tot["max_width"], width)
    tot["max_height"] = max(tot["max_height"], height)
    tot["max_blocks"] = max(tot["max_blocks"], blocks)
    return nmcu, out_bytes + width * height * 3


def pack_headers(hdrs, data_offs, data_ends, subseq_bits, scales=None, dtype=HEADER_DTYPE):
    """Header records + workspace totals for a batch of device-kind headers.
    dtype=HEADER_ANY_DTYPE: the four-component and `layout` headers of one odic_jpeg_any_decode /
    odic_jpeg_any_decode_scaled call; their output offsets are rounded up to multiples of 4, which lets the colour
    kernel store whole words, and with scales the output is placed by `scaled_size` and the planes by
    `scaled_plane_bytes`.  The table count, the rounding and the planes follow from the dtype's fields.
    data_offs / data_ends: byte range of each image's entropy data (SOS end .. blob end) inside the batch's data
    buffer.  scales: 1, 2, 4 or 8 per image (None: all 1), the draft scale its output is placed for.
    → (np array of `dtype` [n], dict of batch totals / maxima, list of output byte offsets, output bytes)."""
    n = len(hdrs)
    rec = np.zeros(n, dtype)
    words = _per_component(dtype)
    ndc = dtype["lut"].shape[0] // 2                  # DC tables 0 .. ndc - 1, AC tables behind them
    tot = dict(total_scan_bytes=0, total_intervals=0, total_units=0, total_blocks=0, total_plane_bytes=0,
               max_units=1, max_intervals=1, max_width=1, max_height=1, max_blocks=1, max_scan_bytes=1)
    out_offs, out_bytes = [], 0
    for k, h in enumerate(hdrs):
        r = rec[k]
        scan = data_ends[k] - data_offs[k]
        nint = n_intervals(h)
        units = -(-scan * 8 // subseq_bits) + nint
        if words:
            out_bytes = (out_bytes + 3) // 4 * 4
        nmcu, out_bytes = _place_image(r, h, tot, out_offs, out_bytes, scales[k] if scales else 1)
        r["data_off"], r["data_end"], r["scan_off"] = data_offs[k], data_ends[k], tot["total_scan_bytes"]
        r["int_off"], r["unit_off"] = tot["total_intervals"], tot["total_units"]
        r["restart"] = h.restart_interval or nmcu
        r["n_intervals"], r["n_units"] = nint, units
        for c in range(h.ncomp):                      # a gray frame: DC table 0, AC table 3, the rest stays zero
            for t, tab in ((c, h.dc_tables[c]), (ndc + c, h.ac_tables[c])):
                lut, mc, vo, hv = device_tables(tab)
                r["lut"][t], r["maxcode"][t], r["valoff"][t], r["huffval"][t] = lut, mc, vo, hv
        tot["total_scan_bytes"] += (scan + 3) // 4 * 4 + 16
        tot["total_intervals"] += nint + 1
        tot["total_units"] += units
        tot["max_units"] = max(tot["max_units"], units)
        tot["max_intervals"] = max(tot["max_intervals"], nint)
        tot["max_scan_bytes"] = max(tot["max_scan_bytes"], scan)
    if (tot["total_intervals"] >= 2 ** 31 or tot["total_units"] >= 2 ** 31
            or tot["max_scan_bytes"] > MAX_SCAN_BYTES):
        raise RuntimeError("JPEG batch too large for one decode call")
    return rec, tot, out_offs, out_bytes


# ---------------------------------------------------------------------------------------------------------------
# Progressive files (SOF2): `parse` turns them away with reason "SOF2"; `parse_progressive` reads the whole scan
# script and either understands it completely or says "host" with a reason.
#
# device  8-bit SOF2 Huffman, three YCbCr components under the rules of `parse`, any scan script libjpeg accepts
#         without a warning and that leaves every coefficient of every component at full precision by EOI
#         (libjpeg's inter-block smoothing only runs for incomplete scripts), DHT / DRI redefined between scans,
#         at most MAX_SCANS scans; under non_rgb="convert" also one component (sampling GRAY), whose scans, the DC scans
#         included, are all non-interleaved over the block raster
# host    everything else: bogus progressions, AC before DC, an incomplete script, DQT or any other marker
#         between scans, DNL, a scan cut short or a missing EOI, more than MAX_SCANS scans
# ---------------------------------------------------------------------------------------------------------------
MAX_SCANS = 64                     # ODIC_JPEG_MAX_SCANS: libjpeg's standard script has 10; arbitrary ones rarely more

# odic_jpeg_prog_header / odic_jpeg_scan / odic_jpeg_table (include/odic_hip.h), field for field
PROG_HEADER_DTYPE = np.dtype([
    ("out_off", "<i8"), ("coef_off", "<i8"), ("plane_off", "<i8"),
    ("width", "<i4"), ("height", "<i4"), ("sampling", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"),
    ("n_intervals", "<i4"), ("qt", "<u2", (3, 64)),
], align=True)
# odic_jpeg_prog_header_any: odic_jpeg_prog_header's prefix with `color` where `sampling` is, then the frame
PROG_HEADER_ANY_DTYPE = np.dtype([
    ("out_off", "<i8"), ("coef_off", "<i8"), ("plane_off", "<i8"),
    ("width", "<i4"), ("height", "<i4"), ("color", "<i4"), ("mcus_x", "<i4"), ("mcus_y", "<i4"),
    ("n_intervals", "<i4"), ("ncomp", "<i4"), ("pad", "<i4"), ("h", "<i4", (4,)), ("v", "<i4", (4,)),
    ("qt", "<u2", (4, 64)),
], align=True)
SCAN_DTYPE = np.dtype([
    ("data_off", "<i8"), ("data_end", "<i8"), ("scan_off", "<i8"),
    ("image", "<i4"), ("int_off", "<i4"), ("n_intervals", "<i4"), ("restart", "<i4"), ("n_units", "<i4"),
    ("blocks_w", "<i4"), ("comp_mask", "<i4"), ("ss", "<i4"), ("se", "<i4"), ("ah", "<i4"), ("al", "<i4"),
    ("level", "<i4"), ("table", "<i4", (3,)), ("pad", "<i4"),
], align=True)
TABLE_DTYPE = np.dtype([
    ("lut", "<u2", (512,)), ("maxcode", "<i4", (18,)), ("valoff", "<i4", (18,)), ("huffval", "u1", (256,)),
], align=True)


@dataclass
class ProgScan:
    comps: list                    # frame component indices, in frame order
    ss: int
    se: int
    ah: int
    al: int
    restart_interval: int          # DRI in effect for this scan (0: none)
    dc_tables: list                # HuffTable per component of a first DC scan, else None
    ac_table: object               # HuffTable of an AC scan, else None
    data_offset: int               # entropy-coded bytes [data_offset, data_end) of the file;
    data_end: int                  # data_end is the first marker that is neither stuffing nor RSTn
    level: int = 1                 # dependency level (1-based)
    n_units: int = 0               # what the scan walks: MCUs (interleaved) or the component's own blocks
    blocks_w: int = 0              # blocks per row of that component's raster (single-component scans)

    @property
    def n_intervals(self):
        return -(-self.n_units // (self.restart_interval or self.n_units))


@dataclass
class ProgHeader(JpegHeader):
    scans: list = field(default_factory=list)

    @property
    def n_levels(self):
        return max((s.level for s in self.scans), default=0)


def marker_positions(blob) -> np.ndarray:
    """Offsets of every 0xFF that is followed by something other than 0x00 (stuffing), RSTn or another 0xFF: inside
    entropy-coded data these are exactly the markers that end a scan.  Vectorised over the whole file."""
    a = np.frombuffer(blob, np.uint8)
    ff = np.flatnonzero(a[:-1] == 0xFF)                  # few: one byte in some hundreds
    nx = a[ff + 1]
    return ff[(nx != 0) & (nx != 0xFF) & ((nx & 0xF8) != 0xD0)]


def parse_progressive(blob, non_rgb: str = "black", cmyk: str = "host", layouts: str = "common") -> ProgHeader:
    """The whole scan script of a progressive file → ProgHeader of kind DEVICE, or HOST with a reason (BLACK for
    one and four components, as `parse`; under non_rgb="convert" a one-component frame is a device kind whose scans
    are all non-interleaved, and a four-component one is HOST); never raises on a file's content.
    cmyk="device" (with non_rgb="convert" only): a four-component SOF2 frame under `_frame4`'s rules is a device kind
    with ncomp 4, comp_hv and `ycck`.  layouts="all": a three-component SOF2 frame that the common rules turn away for
    its sampling or colour space and `_frame3_any` admits is one with `layout` set, comp_hv and `rgb`.  Both are read
    by odic_jpeg_decode_progressive_any (`pack_progressive(..., dtype=PROG_HEADER_ANY_DTYPE)`); the scan-script rules
    are the same, for up to four components.  A frame with more than MAX_MCU_BLOCKS blocks per MCU stays HOST even
    where none of its interleaved scans exceeds libjpeg's limit.  With the defaults the result is what it is without
    the keywords."""
    check_non_rgb(non_rgb)
    check_cmyk(cmyk, non_rgb)
    check_layouts(layouts)
    try:
        return _parse_progressive(bytes(blob), non_rgb, cmyk, layouts)
    except _Bad as e:
        return ProgHeader(HOST, reason=str(e))
    except (IndexError, ValueError) as e:
        return ProgHeader(HOST, reason=f"malformed: {e}")


def _parse_progressive(b, non_rgb="black", cmyk="host", layouts="common") -> ProgHeader:
    w = _Walker(b)
    hd = coef_bits = marks = None                  # set at the first SOS; coef_bits: [3][64] current Al of every
    for s in w.scans(script=True):                 # coefficient, -1: not yet sent (lists)
        if hd is None:
            hd = _frame(w, ProgHeader, (0xC2,), distinct_ids=True, non_rgb=non_rgb, cmyk=cmyk, layouts=layouts)
            hd.app1 = w.app1
            if hd.kind != DEVICE:
                return hd
            coef_bits = [[-1] * 64 for _ in range(hd.ncomp)]
            marks = marker_positions(b)
        if len(hd.scans) >= MAX_SCANS:
            raise _Bad(f"more than {MAX_SCANS} scans")
        sc = _progressive_scan(hd, s, w.dht, w.dri, coef_bits)
        k = int(np.searchsorted(marks, w.i))
        if k >= len(marks):
            raise _Bad("truncated scan")
        sc.data_offset, sc.data_end = w.i, int(marks[k])
        if sc.data_end - sc.data_offset > MAX_SCAN_BYTES:
            raise _Bad("scan longer than the device decoder's bit positions allow")
        hd.scans.append(sc)
        w.i = sc.data_end                          # the walk goes on at the marker that closed the scan
    if any(any(row) for row in coef_bits):
        raise _Bad("incomplete scan script")             # libjpeg smooths across blocks: not a plain decode
    _dependency_levels(hd.scans)
    return hd


def _progressive_scan(hd, s, dht, dri, coef_bits) -> ProgScan:
    """One SOS header under libjpeg's rules (jdmarker.c get_sos, jdphuff.c start_pass_phuff_decoder): whatever
    makes libjpeg warn goes to the host."""
    ns = s[0] if len(s) >= 1 else 0
    if ns < 1 or ns > (4 if hd.ncomp == 4 else 3) or len(s) != 1 + 2 * ns + 3:
        raise _Bad("bad SOS")
    sel = [(s[1 + 2 * k], s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15) for k in range(ns)]
    try:
        comps = [hd.comp_ids.index(x[0]) for x in sel]
    except ValueError:
        raise _Bad("scan names an unknown component") from None
    if comps != sorted(set(comps)):
        raise _Bad("scan component order")
    ss, se, ah, al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15
    if ss == 0:
        if se != 0:
            raise _Bad("bogus progression: DC scan with Se > 0")
    elif se < ss or se > 63 or ns != 1:
        raise _Bad("bogus progression: AC band")
    if al > 13 or (ah != 0 and al != ah - 1):
        raise _Bad("bogus progression: successive approximation")
    for c in comps:
        if ss != 0 and coef_bits[c][0] < 0:
            raise _Bad("AC scan before DC")
        have = coef_bits[c][ss:se + 1]
        if have.count(ah if ah else -1) + (0 if ah else have.count(0)) != len(have):
            raise _Bad("bogus progression: Ah does not continue the previous scan")
        coef_bits[c][ss:se + 1] = [al] * len(have)
    dcs, ac = [None] * ns, None
    if ss == 0 and ah == 0:
        for k in range(ns):
            if (0, sel[k][1]) not in dht:
                raise _Bad("missing DHT")
            dcs[k] = dht[(0, sel[k][1])]
    elif ss != 0:
        if (1, sel[0][2]) not in dht:
            raise _Bad("missing DHT")
        ac = dht[(1, sel[0][2])]
    sc = ProgScan(comps, ss, se, ah, al, dri, dcs, ac, 0, 0)
    if ns > 1:
        sc.n_units = hd.mcus_x * hd.mcus_y
    else:
        h, v = hd.comp_hv[comps[0]]
        hmax, vmax = max(a for a, _ in hd.comp_hv), max(b for _, b in hd.comp_hv)
        sc.blocks_w = -(-(-(-hd.width * h // hmax)) // 8)
        sc.n_units = sc.blocks_w * -(-(-(-hd.height * v // vmax)) // 8)
    return sc


def _dependency_levels(scans):
    """level = 1 + the highest level of an earlier scan that shares a component and overlaps its band (DC scans are
    band 0).  An AC scan also waits for the first DC scan of its component, the order libjpeg insists on.  Scans of
    one level touch disjoint coefficients and decode concurrently."""
    for k, sc in enumerate(scans):
        lvl = 0
        for prev in scans[:k]:
            if not set(prev.comps) & set(sc.comps):
                continue
            if (prev.ss <= sc.se and sc.ss <= prev.se) or (sc.ss > 0 and prev.ss == 0 and prev.ah == 0):
                lvl = max(lvl, prev.level)
        sc.level = lvl + 1


def pack_progressive(hdrs, blob_offs, scales=None, dtype=PROG_HEADER_DTYPE):
    """Header, scan and table records + batch totals for progressive headers whose files start at blob_offs inside
    the batch's data buffer.  Scans are sorted by level (stable), which is how odic_jpeg_decode_progressive walks
    them.  scales: as `pack_headers`.  dtype=PROG_HEADER_ANY_DTYPE: the headers of one odic_jpeg_decode_progressive_any
    / odic_jpeg_decode_progressive_any_scaled call (`parse_progressive` with cmyk="device" / layouts="all"): output
    offsets rounded up to multiples of 4 and planes placed as `pack_headers` does for its word-storing kinds, and the
    fourth DC table index of a scan in its `pad` word.
    → (headers `dtype` [n], scans SCAN_DTYPE [m], tables TABLE_DTYPE [t], totals dict with
    level_first / level_intervals lists, output byte offsets, output bytes)."""
    n = len(hdrs)
    rec = np.zeros(n, dtype)
    own = _per_component(dtype)
    tot = dict(total_scan_bytes=0, total_intervals=0, total_blocks=0, total_plane_bytes=0, max_width=1, max_height=1,
               max_blocks=1)
    tables, table_ix, flat = [], {}, []
    out_offs, out_bytes = [], 0

    def table(t):
        key = (bytes(t.bits), bytes(t.vals))
        if key not in table_ix:
            table_ix[key] = len(tables)
            tables.append(device_tables(t))
        return table_ix[key]

    for k, h in enumerate(hdrs):
        if own:
            out_bytes = (out_bytes + 3) // 4 * 4
        _, out_bytes = _place_image(rec[k], h, tot, out_offs, out_bytes, scales[k] if scales else 1)
        rec[k]["n_intervals"] = sum(s.n_intervals for s in h.scans)
        flat += [(s.level, k, s) for s in h.scans]
    flat.sort(key=lambda x: x[0])
    srec = np.zeros(len(flat), SCAN_DTYPE)
    n_levels = flat[-1][0] if flat else 0
    level_first, level_intervals = [0] * (n_levels + 1), [1] * n_levels
    for j, (lvl, k, s) in enumerate(flat):
        r = srec[j]
        nbytes = s.data_end - s.data_offset
        r["data_off"], r["data_end"] = blob_offs[k] + s.data_offset, blob_offs[k] + s.data_end
        r["scan_off"], r["int_off"] = tot["total_scan_bytes"], tot["total_intervals"]
        r["image"], r["n_intervals"], r["restart"] = k, s.n_intervals, s.restart_interval or s.n_units
        r["n_units"], r["blocks_w"] = s.n_units, s.blocks_w
        r["comp_mask"] = sum(1 << c for c in s.comps)
        r["ss"], r["se"], r["ah"], r["al"], r["level"] = s.ss, s.se, s.ah, s.al, lvl
        r["table"] = -1
        if own:
            r["pad"] = -1
        for q, t in enumerate(s.dc_tables):
            if t is not None and q == 3:
                r["pad"] = table(t)
            elif t is not None:
                r["table"][q] = table(t)
        if s.ac_table is not None:
            r["table"][0] = table(s.ac_table)
        tot["total_scan_bytes"] += (nbytes + 3) // 4 * 4 + 16
        tot["total_intervals"] += s.n_intervals + 1
        level_first[lvl] = j + 1
        level_intervals[lvl - 1] = max(level_intervals[lvl - 1], s.n_intervals)
    for l in range(1, n_levels + 1):                     # levels without a scan cannot occur, but keep it monotonic
        level_first[l] = max(level_first[l], level_first[l - 1])
    trec = np.zeros(max(len(tables), 1), TABLE_DTYPE)
    for q, (lut, mc, vo, hv) in enumerate(tables):
        trec[q]["lut"], trec[q]["maxcode"], trec[q]["valoff"], trec[q]["huffval"] = lut, mc, vo, hv
    if tot["total_intervals"] >= 2 ** 31 or n_levels > MAX_SCANS:
        raise RuntimeError("JPEG batch too large for one decode call")
    tot.update(n_scans=len(flat), n_tables=len(tables), n_levels=n_levels, level_first=level_first,
               level_intervals=level_intervals)
    return rec, srec, trec, tot, out_offs, out_bytes


def pad256(n: int) -> int:
    return (n + 255) // 256 * 256


#: The device groups of one decode, in the order they are laid out: kind → (header dtype, packed by `pack_progressive`).
#: "base" / "prog": the common record family (`parse` / `parse_progressive`); "own" / "pany": the per-component one
#: (cmyk="device" / layouts="all"), three- and four-component files together in input order.
GROUP_KINDS = {"base": (HEADER_DTYPE, False), "prog": (PROG_HEADER_DTYPE, True),
               "own": (HEADER_ANY_DTYPE, False), "pany": (PROG_HEADER_ANY_DTYPE, True)}
COMMON_KINDS = ("base", "prog")


@dataclass
class GroupPlan:
    """One device group of a `BatchPlan`: the files of one decode call."""
    kind: str                      # a key of GROUP_KINDS
    n: int                         # images
    first: int                     # index of its first image in the plan's image order (scales, out_offs, status)
    tot: dict                      # the batch totals of `pack_headers` / `pack_progressive`
    offs: tuple                    # staging offsets of its record sections: (headers,) or (headers, scans, tables)
    out_off: int                   # where its part of the RGB output starts ...
    out_bytes: int                 # ... and its bytes


@dataclass
class BatchPlan:
    """One decode batch in the staging buffer that is uploaded in one copy (256-aligned record sections in the order
    baseline headers, progressive headers / scans / tables, scales, then the records of every later group; then the
    files in group order) and in the output."""
    sections: list                 # [(staging offset, record array)], by offset
    data_off: int                  # the data area: what the records' data_off / data_end count from
    blobs: list                    # [(staging offset, uint8 array)] of every file, in group order
    total: int                     # staging bytes
    groups: list                   # GroupPlan of every group that has files, in GROUP_KINDS order
    scale_off: int                 # staging offset of int32 scale_log2 [images]; None when every scale is 1
    out_offs: list                 # byte offset of every image in the RGB output, in group order
    coef_off: list                 # first coefficient block of every "prog" file, then their total

    def group(self, kind):
        return next((g for g in self.groups if g.kind == kind), None)

    # the two common groups by their earlier names: totals (None without files), the progressive record offsets, and the
    # bytes of the contiguous output they share (the progressive part starts at out_bytes)
    tot = property(lambda self: getattr(self.group("base"), "tot", None))
    ptot = property(lambda self: getattr(self.group("prog"), "tot", None))
    prog_off = property(lambda self: getattr(self.group("prog"), "offs", None))
    out_bytes = property(lambda self: getattr(self.group("base"), "out_bytes", 0))
    pout_bytes = property(lambda self: getattr(self.group("prog"), "out_bytes", 0))

    def fill(self, host):
        """Write the sections and the files into the uint8 array `host` of at least `total` bytes."""
        for o, a in self.sections + self.blobs:
            host[o:o + a.nbytes] = a.view(np.uint8)


def plan_device_batch(groups, subseq_bits, scales) -> BatchPlan:
    """The layout of one device decode.  groups: [(kind, headers, files as bytes)] in GROUP_KINDS order, each the
    DEVICE-kind results of `parse` / `parse_progressive` that `plan_routes` sorted into that kind; a group without files
    may be left out or be empty.  scales: the draft scale of every image in group order; a list that ends early means
    scale 1 for the rest.  Host arithmetic only: this is what keeps every offset the kernels follow inside the upload.
    Every group is placed by one rule: its record sections (256-aligned) behind those of the groups before it, its files
    behind theirs in the data area, its output behind theirs — the two common groups share one contiguous output,
    every later group starts at the next multiple of 256.  The int32 scale_log2 section lies behind the common groups'
    records and holds those two groups, or, where a later group has a scale above 1, every image: group g's entries
    start at 4 · g.first.  A plan of common groups alone does not depend on there being other kinds."""
    groups = [(kind, list(hdrs), list(blobs)) for kind, hdrs, blobs in groups if len(hdrs)]
    kinds = [kind for kind, _, _ in groups]
    if kinds != [kind for kind in GROUP_KINDS if kind in kinds]:
        raise ValueError(f"groups must be distinct kinds in the order {tuple(GROUP_KINDS)}, not {kinds}")
    n_all = sum(len(hdrs) for _, hdrs, _ in groups)
    n_common = sum(len(hdrs) for kind, hdrs, _ in groups if kind in COMMON_KINDS)
    scales = list(scales)[:n_all]
    scales += [1] * (n_all - len(scales))
    if all(s == 1 for s in scales[n_common:]):           # the section then holds the common groups, as without the rest
        scales = scales[:n_common]
    log2 = np.asarray([s.bit_length() - 1 for s in scales], np.int32) if any(s > 1 for s in scales) else None
    sections, plans, files, out_offs, coef_off = [], [], [], [], []
    pos = first = data_end = out_end = 0
    scale_off = None

    def section(a):
        nonlocal pos
        sections.append((pos, a))
        pos += pad256(a.nbytes)
        return sections[-1][0]

    for kind, hdrs, blobs in groups:
        dtype, progressive = GROUP_KINDS[kind]
        common = kind in COMMON_KINDS
        if not common and log2 is not None and scale_off is None:
            scale_off = section(log2)
        n = len(hdrs)
        starts = np.cumsum([data_end] + [len(b) for b in blobs]).tolist()               # inside the data area
        group_scales = scales[first:first + n] or None
        if progressive:
            *recs, tot, offs, nbytes = pack_progressive(hdrs, starts[:-1], group_scales, dtype)
        else:
            *recs, tot, offs, nbytes = pack_headers(hdrs, [o + h.data_offset for o, h in zip(starts, hdrs)],
                                                    starts[1:], subseq_bits, group_scales, dtype)
        out_off = out_end if common else pad256(out_end)
        plans.append(GroupPlan(kind, n, first, tot, tuple(section(a) for a in recs), out_off, nbytes))
        out_offs += [out_off + o for o in offs]
        files += [(o, np.frombuffer(b, np.uint8)) for o, b in zip(starts, blobs)]
        if kind == "prog":
            coef_off = [int(x) for x in recs[0]["coef_off"]] + [int(tot["total_blocks"])]
        first, data_end, out_end = first + n, starts[-1], out_off + nbytes
    if log2 is not None and scale_off is None:
        scale_off = section(log2)
    return BatchPlan(sections, pos, [(pos + o, a) for o, a in files], pos + data_end, plans, scale_off, out_offs,
                     coef_off)
