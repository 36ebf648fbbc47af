"""A progressive (SOF2) JPEG writer for three or four components at any per-component sampling (h, v), built from the
pieces of jpeg_writer (`_ScanCoder`'s four coding procedures, `Scan`, the table builders) and the coefficient maker and
header styles of jpeg_layout_writer: the files Pillow's encoder cannot write — progressive 4:4:0, 4:1:1, 4:1:0, a
component 0 that is not the largest, RGB-stored files, Photoshop's four-component layout — under any scan script.
Pillow is the oracle for what the bytes mean; the writer need agree with no encoder."""
from collections import Counter

import numpy as np

from jpeg_layout_writer import HEADER_STYLES, _seg, component_coefficients
from jpeg_writer import Scan, _Bits, _ScanCoder, check_table, table_codes, table_from_frequencies
from on_device_image_captioning_amd.jpeg import NATURAL_ORDER

#: four components: style → (APPn segments, component ids)
HEADER_STYLES4 = {
    "adobe0": ([(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")], (1, 2, 3, 4)),
    "adobe2": ([(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x02")], (1, 2, 3, 4)),
    "bare": ([], (1, 2, 3, 4)),
}


def frame_mcus(width, height, hv):
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    return -(-width // (8 * hmax)), -(-height // (8 * vmax))


def component_raster(width, height, hv, c):
    """(blocks per row, block rows) of component c's own raster: what a non-interleaved scan walks (T.81 A.2.2)."""
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    h, v = hv[c]
    return -(-(-(-width * h // hmax)) // 8), -(-(-(-height * v // vmax)) // 8)


def raster_to_mcu_order(width, height, hv, c):
    """For every block of component c's own raster, row by row: its index in the component's MCU-ordered array."""
    hh, vv = hv[c]
    mcus_x, _ = frame_mcus(width, height, hv)
    bw, bh = component_raster(width, height, hv, c)
    by, bx = np.mgrid[0:bh, 0:bw]
    return (((by // vv) * mcus_x + bx // hh) * (hh * vv) + (by % vv) * hh + bx % hh).reshape(-1)


def zigzag_coefficients(img, hv, q):
    """`component_coefficients` of the picture → (per component int64 [mcus · h · v, 64] in zig-zag order, DC as its
    value; the natural-order arrays as `write_jpeg3` takes them; (mcus_x, mcus_y))."""
    coefs, mcus = component_coefficients(img, hv, q)
    return [c.reshape(-1, 64)[:, NATURAL_ORDER] for c in coefs], coefs, mcus


class _AnyScanCoder(_ScanCoder):
    """`_ScanCoder` with the frame given as per-component (h, v): only the geometry of the constructor differs, the
    coding procedures are the base class's.  DC and AC table ids default to the component's index."""

    def __init__(self, sc, width, height, hv, coefs):
        self.sc, self.tok = sc, []
        self.eob_runs, self.zrl = [], 0
        mx, my = frame_mcus(width, height, hv)
        if len(sc.comps) > 1:
            self.n_units = mx * my                        # the frame's MCUs, whichever components the scan names
        else:
            self.order = raster_to_mcu_order(width, height, hv, sc.comps[0])
            self.n_units = len(self.order)
        self.R = sc.restart if 0 < sc.restart < self.n_units else self.n_units
        if sc.ss == 0:
            ids = tuple(sc.ids) if sc.ids is not None else tuple(sc.comps)
            self.keys = {c: (0, i) for c, i in zip(sc.comps, ids)}
        else:
            self.key = (1, sc.ids if sc.ids is not None else sc.comps[0])
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
                            per = hv[c][0] * hv[c][1]
                            blocks += [(c, u * per + j) for j in range(per)]
                (self.dc_first if sc.ah == 0 else self.dc_refine)(blocks, coefs)
            else:
                (self.ac_first if sc.ah == 0 else self.ac_refine)(units, coefs[sc.comps[0]])


def write_progressive_any(width, height, hv, coefs, q, script, style="jfif", cut_last=None):
    """One progressive file → bytes.  hv: [(h, v)] of the three or four components; coefs: per component int64
    [mcus · h · v, 64], zig-zag order, MCU by MCU, every entry the final quantised value (`zigzag_coefficients`); q: the
    flat quantiser; script: [jpeg_writer.Scan]; style: a key of HEADER_STYLES (three components) or HEADER_STYLES4.
    Every scan gets optimal tables from its own symbol counts, defined in front of it; DRI wherever the interval
    changes.  cut_last=(n, marker): the last scan's data is cut after n bytes and the two marker bytes put there, the
    rest of the scan dropped (a stream that is wrong on purpose)."""
    n = len(hv)
    segs, ids = (HEADER_STYLES if n == 3 else HEADER_STYLES4)[style]
    coefs = [np.asarray(c, np.int64) for c in coefs]
    mx, my = frame_mcus(width, height, hv)
    for c, (h, v) in zip(coefs, hv):
        assert c.shape == (mx * my * h * v, 64), (c.shape, (mx * my * h * v, 64))
    out = bytearray(b"\xff\xd8" + b"".join(_seg(m, p) for m, p in segs))
    out += _seg(0xDB, bytes([0]) + bytes([q] * 64))
    out += _seg(0xC2, bytes([8, height >> 8, height & 255, width >> 8, width & 255, n]) +
                b"".join(bytes([ids[c], (h << 4) | v, 0]) for c, (h, v) in enumerate(hv)))
    live, dri = {}, 0
    for k, sc in enumerate(script):
        comps = tuple(sc.comps)
        assert comps and list(comps) == sorted(set(comps)) and all(0 <= c < n for c in comps)
        assert sc.ss == 0 or len(comps) == 1
        coder = _AnyScanCoder(sc, width, height, hv, coefs)
        if sc.ss == 0 and sc.ah == 0:
            keys = sorted(set(coder.keys.values()))
        elif sc.ss:
            keys = [coder.key]
        else:
            keys = []
        tables = {}
        for key in keys:
            t = table_from_frequencies(Counter(tok[2] for tok in coder.tok if tok[0] == "s" and tok[1] == key))
            check_table(t)
            tables[key] = (list(t[0]), bytes(t[1]))
        for key in keys:
            if live.get(key) != tables[key]:
                out += _seg(0xC4, bytes([(key[0] << 4) | key[1]]) + bytes(tables[key][0]) + tables[key][1])
        live.update(tables)
        if sc.restart != dri:
            out += _seg(0xDD, bytes([sc.restart >> 8, sc.restart & 255]))
            dri = sc.restart
        codes = {key: table_codes(t) for key, t in tables.items()}
        scan, bw, n_int = bytearray(), _Bits(), 0
        for tok in coder.tok:
            if tok[0] == "s":
                code, length = codes[tok[1]][tok[2]]
                bw.put(code, length)
            elif tok[0] == "b":
                bw.put(tok[1], tok[2])
            elif tok[0] == "c":
                for bit in tok[1]:
                    bw.put(bit, 1)
            else:
                bw.flush(True)
                scan += bw.out + bytes([0xFF, 0xD0 + n_int % 8])
                n_int += 1
                bw = _Bits()
        bw.flush(True)
        scan += bw.out
        if cut_last is not None and k == len(script) - 1:
            scan = scan[:cut_last[0]] + bytes([0xFF, cut_last[1]])
        sos = bytes([len(comps)])
        for c in comps:
            sos += bytes([ids[c], ((coder.keys[c][1] if sc.ss == 0 else 0) << 4) | (coder.key[1] if sc.ss else 0)])
        out += _seg(0xDA, sos + bytes([sc.ss, sc.se, (sc.ah << 4) | sc.al])) + scan
    return bytes(out + b"\xff\xd9")


# ------------------------------------------------------------------------------------------------------------
# scan scripts for n components; `lead`: the components coded as libjpeg codes luma (0, and K of four)
# ------------------------------------------------------------------------------------------------------------
def _lead(n):
    return (0, 3) if n == 4 else (0,)


def standard_script(n, restart=0):
    """libjpeg's jpeg_simple_progression for YCbCr, extended to n components: K takes luma's scans."""
    S, every = Scan, tuple(range(n))
    lead = _lead(n)
    rest = tuple(c for c in every if c not in lead)
    sc = [S(every, 0, 0, 0, 1, restart)]
    sc += [S((c,), 1, 5, 0, 2, restart) for c in lead]
    sc += [S((c,), 1, 63, 0, 1, restart) for c in reversed(rest)]
    sc += [S((c,), 6, 63, 0, 2, restart) for c in lead]
    sc += [S((c,), 1, 63, 2, 1, restart) for c in lead]
    sc += [S(every, 0, 0, 1, 0, restart)]
    sc += [S((c,), 1, 63, 1, 0, restart) for c in reversed(rest)]
    sc += [S((c,), 1, 63, 1, 0, restart) for c in lead]
    return sc


def separate_dc_script(n):
    """Every scan non-interleaved, the DC scans too (with one refinement), then each component's whole AC band."""
    S = Scan
    return [S((c,), 0, 0, 0, 1) for c in range(n)] + [S((c,), 0, 0, 1, 0) for c in range(n)] + \
        [S((c,), 1, 63, 0, 0) for c in range(n)]


def partial_dc_script(n):
    """A first DC scan that interleaves only components {1, 2} (four components: only {0, 3}), the remaining components
    sent separately; the DC refinement interleaves the other way round; then the AC bands."""
    S = Scan
    pair = (0, 3) if n == 4 else (1, 2)
    rest = tuple(c for c in range(n) if c not in pair)
    sc = [S(pair, 0, 0, 0, 1)] + [S((c,), 0, 0, 0, 1) for c in rest]
    sc += [S(rest, 0, 0, 1, 0)] + [S((c,), 0, 0, 1, 0) for c in pair]
    return sc + [S((c,), 1, 63, 0, 0) for c in range(n)]


def split_refine_script(n):
    """AC bands split at 1-5 / 6-63, each with two successive-approximation refinements (Al 2 → 1 → 0)."""
    S = Scan
    sc = [S(tuple(range(n)), 0, 0, 0, 0)]
    for c in range(n):
        for lo, hi in ((1, 5), (6, 63)):
            sc += [S((c,), lo, hi, 0, 2), S((c,), lo, hi, 2, 1), S((c,), lo, hi, 1, 0)]
    return sc


def restart_script(n, r, sub):
    """Restart intervals of r units on the interleaved first DC scan and on the first AC scan of component `sub` (a
    sub-sampled one); the other scans have none, so DRI is redefined between scans."""
    S = Scan
    sc = [S(tuple(range(n)), 0, 0, 0, 0, r)]
    for c in range(n):
        sc += [S((c,), 1, 63, 0, 1, r if c == sub else 0), S((c,), 1, 63, 1, 0)]
    return sc
