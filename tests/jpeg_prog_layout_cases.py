"""Inputs for the progressive per-component-sampling tests (test_jpeg_prog_layouts_host.py, test_jpeg_prog_layouts_gpu.py):
progressive files of three components at the layouts `jpeg.parse_progressive(f, layouts="all")` admits beyond the common
three, RGB-stored ones, and of four components (`cmyk="device"`), from jpeg_prog_layout_writer and from Pillow's own
`save(progressive=True)` of CMYK images.  The oracle is always `np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))`."""
import io

import numpy as np
from PIL import Image

from jpeg_cmyk_cases import PHOTOSHOP_HV, PILLOW_HV, cmyk_image, patch_transform, save_cmyk, write_jpeg4
from jpeg_gray_cases import segments
from jpeg_layout_cases import SIZES, mcu_size, picture
from jpeg_layout_writer import write_jpeg3
from jpeg_prog_layout_writer import (Scan, component_raster, frame_mcus, partial_dc_script, restart_script,
                                     separate_dc_script, split_refine_script, standard_script, write_progressive_any,
                                     zigzag_coefficients)

#: name → ([(h, v)] per component, header style).  Three components: styles of jpeg_layout_writer.HEADER_STYLES; four:
#: jpeg_prog_layout_writer.HEADER_STYLES4 (adobe0 / bare: CMYK as stored, adobe2: YCCK)
LAYOUTS = {
    "440": ([(1, 2), (1, 1), (1, 1)], "jfif"),            # a lossless 90° turn of 4:2:2
    "411": ([(4, 1), (1, 1), (1, 1)], "jfif"),
    "410": ([(4, 2), (1, 1), (1, 1)], "adobe1"),          # ten blocks
    "22-21-21": ([(2, 2), (2, 1), (2, 1)], "jfif"),       # 2x2 luma over 2x1 chroma
    "22-12-12": ([(2, 2), (1, 2), (1, 2)], "bare123"),    # ... and over 1x2 chroma
    "11-21-21": ([(1, 1), (2, 1), (2, 1)], "jfif"),       # a component 0 that is not the largest
    "rgb-bare": ([(1, 1), (1, 1), (1, 1)], "bareRGB"),    # RGB-stored 1x1
    "rgb-adobe0": ([(1, 1), (1, 1), (1, 1)], "adobe0"),
    "c4-11": (PILLOW_HV[0], "adobe0"),                    # Pillow's three four-component layouts
    "c4-21": (PILLOW_HV[1], "adobe2"),
    "c4-22": (PILLOW_HV[2], "adobe0"),
    "photoshop": (PHOTOSHOP_HV, "adobe2"),                # components 0 and 3 at 2x2: ten blocks
}
RGB_STYLES = ("adobe0", "bareRGB")
SCRIPTS = {"separate-dc": separate_dc_script, "partial-dc": partial_dc_script, "split-refine": split_refine_script}
#: the layouts the script variants run on, and the sub-sampled component whose AC scan takes the restart interval
SCRIPT_LAYOUTS = {"440": 1, "410": 2, "11-21-21": 0, "c4-21": 1, "photoshop": 2}


def oracle(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


def source(ncomp, h, w, seed, noise=False):
    return picture(h, w, seed, noise) if ncomp == 3 else cmyk_image(h, w, seed, noise)


class Case:
    """One progressive file with what the writer knows of it, and its baseline twin from the same coefficients."""

    def __init__(self, layout, w, h, seed, script=None, q=6, noise=False):
        self.hv, self.style = LAYOUTS[layout]
        self.ncomp, self.size, self.q = len(self.hv), (w, h), q
        self.route = "device-progressive-cmyk" if self.ncomp == 4 else "device-progressive-layout"
        self.color = self.style == "adobe2" if self.ncomp == 4 else self.style in RGB_STYLES
        self.img = source(self.ncomp, h, w, seed, noise)
        zz, self.coefs, self.mcus = zigzag_coefficients(self.img, self.hv, q)
        self.script = script if script is not None else standard_script(self.ncomp)
        self.blob = write_progressive_any(w, h, self.hv, zz, q, self.script, self.style)

    def baseline(self):
        """The baseline file `write_jpeg3` / `write_jpeg4` write from the same coefficients."""
        if self.ncomp == 3:
            return write_jpeg3(self.img, self.hv, self.style, 0, self.q, mcus=self.mcus, coefs=self.coefs)
        return write_jpeg4(self.img, self.hv, transform=2 if self.style == "adobe2" else 0, q=self.q,
                           adobe=self.style != "bare")


class PillowCase:
    """A progressive CMYK file as Pillow's encoder writes it (or its YCCK twin: the transform byte patched)."""

    def __init__(self, sub, w, h, seed, ycck=False):
        f = save_cmyk(cmyk_image(h, w, seed), quality=88, subsampling=sub, progressive=True)
        self.blob = patch_transform(f, 2) if ycck else f
        self.hv, self.ncomp, self.size, self.color = PILLOW_HV[sub], 4, (w, h), ycck
        self.route, self.script = "device-progressive-cmyk", None


def _build():
    cases = {}
    for k, (layout, (hv, _)) in enumerate(LAYOUTS.items()):
        mw, mh = mcu_size(hv)
        for w, h in SIZES + [(2 * mw, 2 * mh)]:           # ... and exactly two MCUs each way
            cases[f"{layout}-{w}x{h}"] = Case(layout, w, h, seed=k + w)
        cases[f"{layout}-noisy"] = Case(layout, 48, 64, seed=50 + k, q=3, noise=True)
    for k, (layout, sub) in enumerate(SCRIPT_LAYOUTS.items()):
        n = len(LAYOUTS[layout][0])
        for name, make in SCRIPTS.items():
            cases[f"{layout}-{name}"] = Case(layout, 17, 33, seed=70 + k, script=make(n))
        for r in (1, 3):
            cases[f"{layout}-dri{r}"] = Case(layout, 48, 64, seed=80 + k + r, script=restart_script(n, r, sub))
    for sub in (0, 1, 2):
        for w, h in ((17, 33), (48, 64)):
            cases[f"pillow-cmyk-sub{sub}-{w}x{h}"] = PillowCase(sub, w, h, seed=90 + sub)
        cases[f"pillow-ycck-sub{sub}-17x33"] = PillowCase(sub, 17, 33, seed=95 + sub, ycck=True)
    return cases


CASES = _build()
KW = {3: dict(layouts="all"), 4: dict(non_rgb="convert", cmyk="device")}       # the keywords that admit a case


def expected_scan(case, sc):
    """(n_units, blocks_w) `parse_progressive` must report for scan `sc` of a writer case."""
    w, h = case.size
    if len(sc.comps) > 1:
        mx, my = frame_mcus(w, h, case.hv)
        return mx * my, 0
    bw, bh = component_raster(w, h, case.hv, sc.comps[0])
    return bw * bh, bw


def _patch_sof(blob, edit):
    (_, _, p, _), = [s for s in segments(blob) if s[0] == 0xC2]
    b = bytearray(blob)
    edit(b, p)
    return bytes(b)


def cut_short(layout="410", w=17, h=33, seed=7):
    """A file whose last AC scan is cut short by a marker placed mid-scan (DNL, which no scan may hold), with the case
    it was cut from: the scan script is complete, the entropy data is not."""
    case = Case(layout, w, h, seed)
    zz, _, _ = zigzag_coefficients(case.img, case.hv, case.q)
    whole = write_progressive_any(w, h, case.hv, zz, case.q, case.script, case.style)
    last = whole.rfind(b"\xff\xda")
    n = len(whole) - 2 - (last + 2 + ((whole[last + 2] << 8) | whole[last + 3]))    # bytes of the last scan's data
    assert n >= 4
    case.blob = write_progressive_any(w, h, case.hv, zz, case.q, case.script, case.style, cut_last=(n // 2, 0xDC))
    return case


def refused():
    """name → (bytes, a word of the HOST reason, keywords of `parse_progressive`)."""
    img = picture(24, 20, seed=5)
    hv = LAYOUTS["440"][0]
    zz, _, _ = zigzag_coefficients(img, hv, 6)
    f440 = write_progressive_any(20, 24, hv, zz, 6, standard_script(3))
    cm = cmyk_image(24, 20, seed=6)
    zz4, _, _ = zigzag_coefficients(cm, PHOTOSHOP_HV, 6)
    S = Scan
    many = [S((0, 1, 2), 0, 0, 0, 0)] + [S((0,), k, k, 0, 0) for k in range(1, 62)] + \
        [S((0,), 62, 63, 0, 0), S((1,), 1, 63, 0, 0), S((2,), 1, 63, 0, 0)]
    assert len(many) == 65
    ac_first = [S((0, 1, 2), 0, 0, 0, 0), S((3,), 1, 63, 0, 0), S((3,), 0, 0, 0, 0)] + \
        [S((c,), 1, 63, 0, 0) for c in range(3)]

    def set_hv(new):
        def edit(b, p):
            for c, (h, v) in enumerate(new):
                b[p + 7 + 3 * c] = (h << 4) | v
        return edit

    def same_ids(b, p):
        b[p + 6 + 3] = b[p + 6]

    return {
        "fractional": (_patch_sof(f440, set_hv([(3, 1), (2, 1), (2, 1)])), "fractional", KW[3]),
        "duplicate ids": (_patch_sof(f440, same_ids), "duplicate", KW[3]),
        "Adobe transform 2 on three": (write_progressive_any(20, 24, hv, zz, 6, standard_script(3), "adobe2"),
                                       "transform 2", KW[3]),
        "incomplete script": (write_progressive_any(20, 24, hv, zz, 6, standard_script(3)[:-1]), "incomplete", KW[3]),
        "65 scans": (write_progressive_any(20, 24, hv, zz, 6, many), "more than 64 scans", KW[3]),
        "AC before DC on component 3": (write_progressive_any(20, 24, PHOTOSHOP_HV, zz4, 6, ac_first, "adobe2"),
                                        "AC scan before DC", KW[4]),
        "13 blocks per MCU": (_patch_sof(write_progressive_any(20, 24, PHOTOSHOP_HV, zz4, 6, standard_script(4), "adobe2"),
                                         set_hv([(2, 2), (2, 2), (1, 1), (2, 2)])), "13 blocks per MCU", KW[4]),
    }
