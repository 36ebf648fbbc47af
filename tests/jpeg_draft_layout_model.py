"""A numpy model of the scaled (draft) decode of JPEGs with per-component sampling, and the files the draft-layout tests
share (test_jpeg_draft_layouts_host.py, test_jpeg_draft_layouts_gpu.py).  The model starts from the quantised
coefficients the writers take and follows libjpeg at 1 / scale: dequantisation, the reduced ISLOW transform of every
component at the size `jpeg.scaled_components` gives it, the upsampling that remains (h2v1 / h1v2 triangle filters while
8 / scale > 1, replication otherwise), then YCbCr → RGB, RGB as stored, or YCCK / CMYK → RGB.  The oracle is always
`Image.open(f); im.draft("RGB", request); im.convert("RGB")`."""
import io

import numpy as np
from PIL import Image

from jpeg_cmyk_cases import PHOTOSHOP_HV, PILLOW_HV, cmyk_image, color_model, write_jpeg4
from jpeg_layout_cases import picture
from jpeg_layout_writer import component_coefficients, write_jpeg3
from jpeg_prog_layout_writer import split_refine_script, standard_script, write_progressive_any
from on_device_image_captioning_amd import jpeg as J
from on_device_image_captioning_amd.jpeg import NATURAL_ORDER
from test_jpeg_draft_host import model_reduced_idct

#: name → ([(h, v)] per component, header style — jpeg_layout_writer.HEADER_STYLES for three components,
#: jpeg_prog_layout_writer.HEADER_STYLES4 for four: adobe0 is CMYK as stored, adobe2 YCCK)
LAYOUTS = {
    "440": ([(1, 2), (1, 1), (1, 1)], "jfif"),
    "411": ([(4, 1), (1, 1), (1, 1)], "jfif"),
    "410": ([(4, 2), (1, 1), (1, 1)], "adobe1"),
    "22-21-21": ([(2, 2), (2, 1), (2, 1)], "jfif"),       # 2x2 luma with 2x1 chroma
    "22-12-12": ([(2, 2), (1, 2), (1, 2)], "bare123"),    # 2x2 luma with 1x2 chroma
    "11-21-21": ([(1, 1), (2, 1), (2, 1)], "jfif"),       # component 0 not the largest
    "rgb-adobe0": ([(1, 1), (1, 1), (1, 1)], "adobe0"),   # RGB-stored by Adobe transform 0
    "rgb-22": ([(2, 2), (1, 1), (1, 1)], "adobe0"),       # ... with sub-sampling
    "cmyk-11": (PILLOW_HV[0], "adobe0"),                  # four components all 1x1
    "ycck-11": (PILLOW_HV[0], "adobe2"),
    "cmyk-21": (PILLOW_HV[1], "adobe0"),                  # component 0 at 2x1
    "ycck-21": (PILLOW_HV[1], "adobe2"),
    "cmyk-22": (PILLOW_HV[2], "adobe0"),                  # component 0 at 2x2
    "ycck-22": (PILLOW_HV[2], "adobe2"),
    "photoshop-cmyk": (PHOTOSHOP_HV, "adobe0"),           # components 0 and 3 at 2x2
    "photoshop-ycck": (PHOTOSHOP_HV, "adobe2"),
}
RGB_STYLES = ("adobe0", "bareRGB")
#: (w, h); none a multiple of the MCU.  3 x 40 and 40 x 3 (at 1/2), 9 x 36 and 36 x 9 (at 1/4): a sub-sampled plane at
#: most two samples across
SIZES = [(17, 33), (48, 64), (93, 67), (3, 40), (40, 3), (9, 36), (36, 9)]
SCALES = (2, 4, 8)
KW = {3: dict(layouts="all"), 4: dict(non_rgb="convert", cmyk="device")}       # the keywords that admit a case


def request_for(size, s):
    """A draft request that makes Pillow pick scale s for an image of `size` (w, h), if the image is large enough."""
    return max(size[0] // s, 1), max(size[1] // s, 1)


def pil_draft_rgb(blob, req):
    """→ (what the host route makes of the file under the draft request, the scale Pillow picked)."""
    im = Image.open(io.BytesIO(blob))
    im.draft("RGB", req)
    scale = im.decoderconfig[0] if im.decoderconfig else 1
    return np.asarray(im.convert("RGB"), dtype=np.uint8), scale


class Case:
    """One picture with its quantised coefficients and the files written from them: baseline (with a restart interval
    where asked) and progressive under a given script."""

    def __init__(self, layout, w, h, seed, restart=0, q=6, noise=False):
        self.layout, (self.hv, self.style) = layout, LAYOUTS[layout]
        self.ncomp, self.size, self.q, self.restart = len(self.hv), (w, h), q, restart
        self.ycck = self.ncomp == 4 and self.style == "adobe2"
        self.rgb = self.ncomp == 3 and self.style in RGB_STYLES
        self.img = picture(h, w, seed, noise) if self.ncomp == 3 else cmyk_image(h, w, seed, noise)
        self.coefs, self.mcus = component_coefficients(self.img, self.hv, q)

    @property
    def kw(self):
        return KW[self.ncomp]

    def baseline(self):
        if self.ncomp == 3:
            return write_jpeg3(self.img, self.hv, self.style, self.restart, self.q, mcus=self.mcus, coefs=self.coefs)
        return write_jpeg4(self.img, self.hv, transform=2 if self.ycck else 0, restart=self.restart, q=self.q)

    def progressive(self, script=None):
        w, h = self.size
        zz = [c.reshape(-1, 64)[:, NATURAL_ORDER] for c in self.coefs]
        script = script if script is not None else standard_script(self.ncomp, self.restart)
        return write_progressive_any(w, h, self.hv, zz, self.q, script, self.style)

    def split_refine(self):
        return self.progressive(split_refine_script(self.ncomp))


def model_planes(case, scale):
    """Per component: the int64 sample plane [mcus_y · v · n, mcus_x · h · n] of the reduced transforms, and
    `jpeg.scaled_components` of the frame."""
    geo = J.scaled_components(case.hv, scale)
    mx, my = case.mcus
    qt = np.full(64, case.q, np.int64)
    planes = []
    for coef, (h, v), (n, _, _) in zip(case.coefs, case.hv, geo):
        pix = model_reduced_idct(coef.reshape(-1, 64), qt, n).astype(np.int64)
        planes.append(pix.reshape(my, mx, v, h, n, n).transpose(0, 2, 4, 1, 3, 5).reshape(my * v * n, mx * h * n))
    return planes, geo


def upsample(P, rh, rv, dw, dh, ow, oh, fancy):
    """jdsample.c on one plane with dw x dh real samples → int64 [oh, ow]: copy; h2v1 (and h2v2, which no admitted frame
    reaches below full size) fancy while the plane is more than two samples wide; h1v2 fancy at every width; replication
    for every other ratio and wherever `fancy` is off (a 1x1 smallest transform)."""
    x, y = np.arange(ow), np.arange(oh)
    if not fancy or (rh, rv) not in ((2, 1), (1, 2)) or (rh == 2 and dw <= 2):
        return P[(y // rv)[:, None], (x // rh)[None, :]]
    if rh == 2:
        c = x >> 1
        cn = np.where(x & 1, np.minimum(c + 1, dw - 1), np.maximum(c - 1, 0))
        a, b = P[:oh][:, c], P[:oh][:, cn]
        return (3 * a + b + 1 + (x & 1)) >> 2
    r = y >> 1
    rn = np.where(y & 1, np.minimum(r + 1, dh - 1), np.maximum(r - 1, 0))
    a, b = P[r][:, :ow], P[rn][:, :ow]
    return (3 * a + b + 1 + (y & 1)[:, None]) >> 2


def model_draft_rgb(case, scale):
    """The scaled decode of the case's coefficients → uint8 [ceil(H / scale), ceil(W / scale), 3]."""
    planes, geo = model_planes(case, scale)
    W, H = case.size
    ow, oh = J.scaled_size(case.size, scale)
    hmax, vmax = max(h for h, _ in case.hv), max(v for _, v in case.hv)
    full = []
    for P, (h, v), (n, rh, rv) in zip(planes, case.hv, geo):
        dw, dh = -(-W * h * n // (hmax * 8)), -(-H * v * n // (vmax * 8))      # jdmaster.c: the downsampled size
        full.append(upsample(P, rh, rv, dw, dh, ow, oh, fancy=scale < 8))
    s = np.stack(full, axis=2)
    if case.ncomp == 4:
        return color_model(s.astype(np.uint8), case.ycck)
    if case.rgb:
        return s.astype(np.uint8)
    y, cb, cr = s[..., 0], s[..., 1] - 128, s[..., 2] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def _build():
    cases = {}
    for k, layout in enumerate(LAYOUTS):
        for j, (w, h) in enumerate(SIZES):
            # a restart interval on one size of every layout (baseline: DRI; progressive: every scan of the script)
            cases[f"{layout}-{w}x{h}"] = Case(layout, w, h, seed=3 * k + j, restart=3 if (w, h) == (48, 64) else 0)
    return cases


CASES = _build()
