"""Inputs for the sampling-layout tests (test_jpeg_layouts_host.py, test_jpeg_layouts_gpu.py): three-component baseline
files at the layouts `jpeg.parse(f, layouts="all")` admits beyond the common three, and RGB-stored ones, all from
jpeg_layout_writer.  The oracle is always `np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))`."""
import io

import numpy as np
from PIL import Image

from jpeg_cmyk_cases import NOISE_AMPLITUDE
from jpeg_gray_cases import segments
from jpeg_layout_writer import component_coefficients, write_jpeg3

#: name → ([(h, v)] of the three components, header style)
LAYOUTS = {
    "440": ([(1, 2), (1, 1), (1, 1)], "jfif"),            # 4:4:0: h1v2 fancy
    "411": ([(4, 1), (1, 1), (1, 1)], "jfif"),            # 4:1:1: 4x1 replication
    "410": ([(4, 2), (1, 1), (1, 1)], "adobe1"),          # 4:1:0: ten blocks
    "22-12-12": ([(2, 2), (1, 2), (1, 2)], "jfif"),       # h2v1 fancy on chroma, two chroma blocks stacked
    "22-21-21": ([(2, 2), (2, 1), (2, 1)], "bare123"),    # h1v2 fancy on chroma, two chroma blocks side by side
    "11-21-21": ([(1, 1), (2, 1), (2, 1)], "jfif"),       # luma upsampled h2v1
    "21-11-21": ([(2, 1), (1, 1), (2, 1)], "bareXYZ"),    # mixed
    "31": ([(3, 1), (1, 1), (1, 1)], "jfif"),             # ratio 3 replication
    "14": ([(1, 4), (1, 1), (1, 1)], "jfif"),             # 1x4 replication
    "rgb-adobe0": ([(1, 1), (1, 1), (1, 1)], "adobe0"),
    "rgb-bare": ([(1, 1), (1, 1), (1, 1)], "bareRGB"),
    "rgb-22": ([(2, 2), (1, 1), (1, 1)], "adobe0"),       # RGB with sub-sampling
}
RGB_STYLES = ("adobe0", "bareRGB")
SIZES = [(1, 1), (3, 5), (7, 9), (17, 33), (48, 64)]      # (w, h); 3x5: every sub-sampled plane is at most 2 wide;
                                                          # 17x33: a multiple of no MCU in either direction


def picture(h, w, seed=0, noise=False):
    """uint8 [h, w, 3]: a smooth gradient per channel, plus uniform noise of ±NOISE_AMPLITUDE when asked."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 9.0 + seed + c) * np.cos(y / 11.0 + 0.7 * c) for c in range(3)], axis=2)
    if noise:
        img = img + rng.uniform(-NOISE_AMPLITUDE, NOISE_AMPLITUDE, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def oracle(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


def mcu_size(hv):
    return 8 * max(h for h, _ in hv), 8 * max(v for _, v in hv)


class Case:
    """One file with what the writer knows of it: the layout, the colour space, the quantiser and the coefficients."""

    def __init__(self, layout, w, h, seed, restart=0, q=6, noise=False):
        self.hv, self.style = LAYOUTS[layout]
        self.rgb, self.q, self.restart, self.size = self.style in RGB_STYLES, q, restart, (w, h)
        img = picture(h, w, seed, noise)
        self.coefs, self.mcus = component_coefficients(img, self.hv, q)
        self.blob = write_jpeg3(img, self.hv, self.style, restart, q, mcus=self.mcus, coefs=self.coefs)


def _build():
    cases = {}
    for k, (layout, (hv, _)) in enumerate(LAYOUTS.items()):
        mw, mh = mcu_size(hv)
        for w, h in SIZES + [(2 * mw, 2 * mh)]:           # ... and one size of whole MCUs
            cases[f"{layout}-{w}x{h}"] = Case(layout, w, h, seed=k + w)
        cases[f"{layout}-noisy"] = Case(layout, 48, 64, seed=50 + k, q=3, noise=True)
    for layout in ("440", "411"):
        for r in (1, 3):
            cases[f"{layout}-dri{r}"] = Case(layout, 48, 64, seed=40 + r, restart=r)
    return cases


CASES = _build()


def patch_sof_hv(blob, hv):
    """The same file with the SOF's sampling bytes set to hv (the entropy data no longer fits: for the parser's eyes)."""
    (_, _, p, _), = [s for s in segments(blob) if s[0] in (0xC0, 0xC1, 0xC2)]
    b = bytearray(blob)
    assert b[p + 5] == 3
    for c, (h, v) in enumerate(hv):
        b[p + 7 + 3 * c] = (h << 4) | v
    return bytes(b)


def refused():
    """name → (bytes, a word of the HOST reason, keywords of `parse`) for files that stay on the host.  A draft request
    is refused by `decode_jpeg`, which leaves `layouts` out of its `parse` calls then: the common rules' reason."""
    img = picture(24, 20, seed=5)
    f440 = write_jpeg3(img, LAYOUTS["440"][0])
    every = dict(layouts="all")
    return {
        "fractional": (patch_sof_hv(f440, [(3, 1), (2, 1), (2, 1)]), "fractional", every),
        "11 blocks": (write_jpeg3(img, [(4, 2), (2, 1), (1, 1)]), "11 blocks per MCU", every),
        "Adobe transform 2": (write_jpeg3(img, LAYOUTS["440"][0], "adobe2"), "transform 2", every),
        "SOF2 at 4:4:0": (write_jpeg3(img, LAYOUTS["440"][0], sof=0xC2), "progressive", every),
        "draft request": (f440, "sampling", {}),
    }
