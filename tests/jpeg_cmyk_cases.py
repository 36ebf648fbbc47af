"""Inputs for the four-component tests (test_jpeg_cmyk_host.py, test_jpeg_cmyk_gpu.py): CMYK JPEGs as Pillow writes them
(all components 1x1, or component 0 at 2x1 / 2x2), byte edits of those (the Adobe transform byte → YCCK, the APP14
segment cut out or replaced by a JFIF APP0, SOF edits that the parser must refuse), and streams from a small
four-component baseline writer for the layout Photoshop uses (components 0 and 3 at 2x2 or 2x1, 1 and 2 at 1x1), which
Pillow cannot write.  The oracle is always `np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))`."""
import io

import numpy as np
from PIL import Image

from jpeg_gray_cases import segments
from jpeg_writer import STD_AC_CHROMA, STD_AC_LUMA, STD_DC_CHROMA, STD_DC_LUMA, _Bits, _dct_matrix, amplitude_bits, \
    block_symbols, table_codes
from on_device_image_captioning_amd.jpeg import NATURAL_ORDER

SIZES = [(1, 1), (7, 9), (17, 33), (48, 64)]          # (w, h): one pixel, partial MCUs on both axes, several MCUs
#: the noisy cases add uniform noise of this amplitude (±) to the gradient; full-range noise also decodes on the device
#: at these qualities, the bound only keeps the dequantised coefficients well inside the IDCT's agreed range
NOISE_AMPLITUDE = 48
PHOTOSHOP_HV = [(2, 2), (1, 1), (1, 1), (2, 2)]       # ten blocks per MCU
PHOTOSHOP_HV_2x1 = [(2, 1), (1, 1), (1, 1), (2, 1)]


def cmyk_image(h, w, seed=0, noise=False):
    """uint8 [h, w, 4]: a smooth gradient per channel, plus noise of ±NOISE_AMPLITUDE when asked."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ch = [128 + 100 * np.sin(x / 9.0 + seed + c) * np.cos(y / 11.0 + 0.7 * c) for c in range(3)]
    ch.append(60 + 50 * np.sin((x + y) / 13.0 + seed))
    img = np.stack(ch, axis=2)
    if noise:
        img = img + rng.uniform(-NOISE_AMPLITUDE, NOISE_AMPLITUDE, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def save_cmyk(img, **kw):
    out = io.BytesIO()
    Image.fromarray(img, "CMYK").save(out, "JPEG", **kw)
    return out.getvalue()


def oracle(blob):
    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"), dtype=np.uint8)


def _segment_of(blob, marker, tag=b""):
    hits = [s for s in segments(blob) if s[0] == marker and blob[s[2]:s[2] + len(tag)] == tag]
    assert len(hits) == 1, (marker, len(hits))
    return hits[0]


def patch_transform(blob, transform):
    """The same file with the transform byte of its Adobe APP14 segment (offset 11 behind the tag) set."""
    _, _, p, n = _segment_of(blob, 0xEE, b"Adobe")
    assert n >= 12
    b = bytearray(blob)
    b[p + 11] = transform
    return bytes(b)


JFIF_APP0 = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"


def replace_app14(blob, by=b""):
    """The same file with its Adobe APP14 segment cut out, or replaced by the segment(s) `by`."""
    _, at, p, n = _segment_of(blob, 0xEE, b"Adobe")
    return blob[:at] + by + blob[p + n:]


def patch_sof_hv(blob, hv):
    """The same file with the SOF's sampling bytes of its four components set to hv [(h, v)] (the entropy data no
    longer fits: for the parser's eyes only)."""
    (_, _, p, _), = [s for s in segments(blob) if s[0] in (0xC0, 0xC1, 0xC2)]
    b = bytearray(blob)
    assert b[p + 5] == 4
    for c, (h, v) in enumerate(hv):
        b[p + 7 + 3 * c] = (h << 4) | v
    return bytes(b)


# ------------------------------------------------------------------------------------------------------------
# a four-component baseline writer: every component with its own sampling, one quantisation table, the standard
# Huffman tables (luma's for components 0 and 3, chroma's for 1 and 2), Adobe APP14 with the given transform
# ------------------------------------------------------------------------------------------------------------
def write_jpeg4(img, hv, transform=2, restart=0, q=6, adobe=True):
    """uint8 [H, W, 4] samples as the file is to store them → bytes.  Components below component 0's sampling are
    box-filtered; edges are replicated up to whole MCUs; float DCT, rounding, a flat quantiser q."""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    hmax, vmax = hv[0]
    assert all(h <= hmax and v <= vmax for h, v in hv)
    mx, my = -(-W // (8 * hmax)), -(-H // (8 * vmax))
    img = np.pad(img, ((0, my * 8 * vmax - H), (0, mx * 8 * hmax - W), (0, 0)), mode="edge")
    d = _dct_matrix()
    blocks = []                                           # per component [mcus, h * v, 64] zig-zag, DC as its value
    for c, (h, v) in enumerate(hv):
        p = img[..., c].reshape(my * 8 * v, vmax // v, mx * 8 * h, hmax // h).mean(axis=(1, 3))
        blk = (p - 128).reshape(my, v, 8, mx, h, 8).transpose(0, 3, 1, 4, 2, 5).reshape(-1, 8, 8)
        f = np.rint(d @ blk @ d.T / q).astype(np.int64).reshape(-1, 64)
        blocks.append(f[:, NATURAL_ORDER].reshape(mx * my, h * v, 64))
    tabs = [(STD_DC_LUMA, STD_AC_LUMA), (STD_DC_CHROMA, STD_AC_CHROMA)]
    tid = [0, 1, 1, 0]
    codes = [(table_codes(dc), table_codes(ac)) for dc, ac in tabs]
    nmcu = mx * my
    R = restart if 0 < restart < nmcu else nmcu
    scan = bytearray()
    for k, m0 in enumerate(range(0, nmcu, R)):
        if m0:
            scan += bytes([0xFF, 0xD0 + (k - 1) % 8])
        bw, pred = _Bits(), [0] * 4
        for m in range(m0, min(m0 + R, nmcu)):
            for c in range(4):
                for blk in blocks[c][m]:
                    blk = blk.copy()
                    blk[0], pred[c] = blk[0] - pred[c], blk[0]
                    for n, (sym, value) in enumerate(block_symbols(blk)):
                        code, length = codes[tid[c]][n > 0][sym]
                        bw.put(code, length)
                        if sym & 15:
                            bw.put(amplitude_bits(value, sym & 15), sym & 15)
        bw.flush(True)
        scan += bw.out

    def seg(marker, payload):
        return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + payload

    out = b"\xff\xd8"
    if adobe:
        out += seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))
    out += seg(0xDB, bytes([0]) + bytes([q] * 64))
    out += seg(0xC0, bytes([8, H >> 8, H & 255, W >> 8, W & 255, 4]) +
               b"".join(bytes([c + 1, (h << 4) | v, 0]) for c, (h, v) in enumerate(hv)))
    for i, (dc, ac) in enumerate(tabs):
        out += seg(0xC4, bytes([i]) + bytes(dc[0]) + bytes(dc[1])) + seg(0xC4, bytes([0x10 | i]) + bytes(ac[0]) + bytes(ac[1]))
    if restart:
        out += seg(0xDD, bytes([restart >> 8, restart & 255]))
    out += seg(0xDA, bytes([4]) + b"".join(bytes([c + 1, (tid[c] << 4) | tid[c]]) for c in range(4)) + b"\x00\x3f\x00")
    return out + bytes(scan) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------------------
# the admitted cases: name → (bytes, comp_hv, ycck)
# ------------------------------------------------------------------------------------------------------------
PILLOW_HV = {0: [(1, 1)] * 4, 1: [(2, 1)] + [(1, 1)] * 3, 2: [(2, 2)] + [(1, 1)] * 3}


def _build():
    cases = {}
    for sub in (0, 1, 2):
        for w, h in SIZES:
            f = save_cmyk(cmyk_image(h, w, seed=sub + w), quality=88, subsampling=sub)
            cases[f"cmyk-sub{sub}-{w}x{h}"] = (f, PILLOW_HV[sub], False)
            cases[f"ycck-sub{sub}-{w}x{h}"] = (patch_transform(f, 2), PILLOW_HV[sub], True)
    plain = save_cmyk(cmyk_image(33, 17, seed=9), quality=88, subsampling=2)
    cases["cmyk-no-app14"] = (replace_app14(plain), PILLOW_HV[2], False)
    cases["cmyk-jfif-no-adobe"] = (replace_app14(plain, JFIF_APP0), PILLOW_HV[2], False)
    for w, h in SIZES:
        cases[f"photoshop-ycck-2x2-{w}x{h}"] = (write_jpeg4(cmyk_image(h, w, seed=20 + w), PHOTOSHOP_HV), PHOTOSHOP_HV, True)
    cases["photoshop-ycck-2x1-17x33"] = (write_jpeg4(cmyk_image(33, 17, seed=31), PHOTOSHOP_HV_2x1), PHOTOSHOP_HV_2x1, True)
    cases["photoshop-ycck-2x1-48x64"] = (write_jpeg4(cmyk_image(64, 48, seed=32), PHOTOSHOP_HV_2x1), PHOTOSHOP_HV_2x1, True)
    cases["photoshop-cmyk-2x2-17x33"] = (write_jpeg4(cmyk_image(33, 17, seed=33), PHOTOSHOP_HV, transform=0), PHOTOSHOP_HV,
                                         False)
    cases["photoshop-cmyk-2x2-no-adobe"] = (write_jpeg4(cmyk_image(33, 17, seed=34), PHOTOSHOP_HV, adobe=False),
                                            PHOTOSHOP_HV, False)
    for r in (1, 3):
        f = save_cmyk(cmyk_image(64, 48, seed=40 + r), quality=88, subsampling=2, restart_marker_blocks=r)
        assert b"\xff\xdd" in f
        cases[f"cmyk-sub2-dri{r}"] = (f, PILLOW_HV[2], False)
        cases[f"ycck-sub0-dri{r}"] = (patch_transform(save_cmyk(cmyk_image(33, 17, seed=42 + r), quality=88, subsampling=0,
                                                                restart_marker_blocks=r), 2), PILLOW_HV[0], True)
        cases[f"photoshop-ycck-2x2-dri{r}"] = (write_jpeg4(cmyk_image(64, 48, seed=44 + r), PHOTOSHOP_HV, restart=r),
                                               PHOTOSHOP_HV, True)
    for sub in (0, 2):
        f = save_cmyk(cmyk_image(64, 48, seed=50 + sub, noise=True), quality=90, subsampling=sub)
        cases[f"cmyk-noisy-sub{sub}"] = (f, PILLOW_HV[sub], False)
        cases[f"ycck-noisy-sub{sub}"] = (patch_transform(f, 2), PILLOW_HV[sub], True)
    cases["photoshop-ycck-noisy"] = (write_jpeg4(cmyk_image(64, 48, seed=55, noise=True), PHOTOSHOP_HV, q=3), PHOTOSHOP_HV,
                                     True)
    return cases


CASES = _build()


def refused():
    """name → (bytes, a word of the HOST reason) for files `parse(..., "convert", cmyk="device")` turns away."""
    base = save_cmyk(cmyk_image(24, 20, seed=5), quality=88)
    return {
        "progressive (SOF2)": (save_cmyk(cmyk_image(24, 20, seed=5), quality=88, progressive=True), "SOF2"),
        "16 blocks per MCU": (patch_sof_hv(base, [(2, 2)] * 4), "16 blocks per MCU"),
        # under the sampling rule an MCU has 4, 7, 10, 13 or 16 blocks (2x2) or up to 8 (2x1): 13 is the first past 10
        "13 blocks per MCU": (patch_sof_hv(base, [(2, 2), (2, 2), (1, 1), (2, 2)]), "13 blocks per MCU"),
        "Adobe transform 1": (patch_transform(base, 1), "transform 1"),
        "Adobe transform 7": (patch_transform(base, 7), "transform 7"),
        "component 0 at 1x2": (patch_sof_hv(base, [(1, 2), (1, 1), (1, 1), (1, 1)]), "sampling"),
        "component 2 at 2x1 under 2x2": (patch_sof_hv(base, [(2, 2), (1, 1), (2, 1), (1, 1)]), "sampling"),
        "duplicate component ids": (_duplicate_ids(base), "duplicate"),
    }


def _duplicate_ids(blob):
    (_, _, p, _), = [s for s in segments(blob) if s[0] == 0xC0]
    b = bytearray(blob)
    b[p + 6 + 3] = b[p + 6]                               # component 1 takes component 0's id
    return bytes(b)


def color_model(planes, ycck):
    """The colour chain on the four upsampled planes as the file stores them, uint8 [H, W, 4] → uint8 [H, W, 3]:
    YCCK → CMYK (libjpeg's table-driven YCbCr → RGB, complemented), Pillow's inversion of every sample, Pillow's
    CMYK → RGB."""
    s = planes.astype(np.int64)
    if ycck:
        y, cb, cr = s[..., 0], s[..., 1] - 128, s[..., 2] - 128
        r = np.clip(y + ((91881 * cr + 32768) >> 16), 0, 255)
        g = np.clip(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255)
        b = np.clip(y + ((116130 * cb + 32768) >> 16), 0, 255)
        s = np.stack([255 - r, 255 - g, 255 - b, s[..., 3]], axis=-1)
    s = 255 - s
    return cmyk_to_rgb_model(s)


def cmyk_to_rgb_model(s):
    s = np.asarray(s, np.int64)
    nk = 255 - s[..., 3:4]
    t = s[..., :3] * nk + 128
    return np.clip(nk - (((t >> 8) + t) >> 8), 0, 255).astype(np.uint8)
