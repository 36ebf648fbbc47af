"""Inputs for the grayscale / non-RGB tests (test_jpeg_gray_host.py, test_jpeg_gray_gpu.py): one-component JPEGs as
Pillow writes them, plain byte edits of those (the SOF's sampling factors, the component id, damaged entropy data), a
CMYK JPEG, PNGs of other modes, and the oracle: `np.asarray(Image.open(f).convert("RGB"))`, after `draft` if asked."""
import io

import numpy as np
from PIL import Image

SIZES = [(1, 1), (7, 9), (8, 8), (9, 17), (37, 53)]        # (w, h): one block, partial blocks on each axis and both, 35
HV_PATCHES = (0x22, 0x21, 0x12, 0x41)                      # sampling factors a one-component SOF may declare
PATCHED_ID = 7

#: kind → Pillow save options.  "noise100" is quality-100 noise; the others are a smooth picture with some texture.
KINDS = {
    "baseline": dict(quality=85),
    "optimize": dict(quality=85, optimize=True),
    "noise100": dict(quality=100),
    "dri1": dict(quality=85, restart_marker_blocks=1),
    "dri3": dict(quality=85, restart_marker_blocks=3),     # 37 x 53: 35 blocks, 12 intervals, RSTn wraps past 7
    "progressive": dict(quality=85, progressive=True),
    "progressive-dri3": dict(quality=85, progressive=True, restart_marker_blocks=3),
}


def gray_image(h, w, seed=0, noise=False):
    rng = np.random.default_rng(seed)
    if noise:
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    img = 128 + 90 * np.sin(x / 5.0 + seed) * np.cos(y / 7.0) + rng.normal(0, 6, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def save_gray(img, **kw):
    out = io.BytesIO()
    Image.fromarray(img, "L").save(out, "JPEG", **kw)
    return out.getvalue()


def gray_file(kind, size, seed=0):
    w, h = size
    return save_gray(gray_image(h, w, seed=seed + w + h, noise=kind == "noise100"), **KINDS[kind])


def cmyk_jpeg(h=24, w=20, seed=5):
    arr = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    out = io.BytesIO()
    Image.fromarray(arr, "CMYK").save(out, "JPEG", quality=90)
    return out.getvalue()


def png(mode, h=19, w=23, seed=3):
    rng = np.random.default_rng(seed)
    if mode == "P":
        im = Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "P")
        im.putpalette(rng.integers(0, 256, 768, dtype=np.uint8).tobytes())
    elif mode == "I;16":
        im = Image.fromarray(rng.integers(0, 65536, (h, w), dtype=np.uint16))
        assert im.mode == "I;16"
    else:
        channels = {"L": (), "LA": (2,), "RGBA": (4,)}[mode]
        im = Image.fromarray(rng.integers(0, 256, (h, w) + channels, dtype=np.uint8), mode)
    out = io.BytesIO()
    im.save(out, "PNG")
    return out.getvalue()


def pil_convert(blob, draft=None):
    """The oracle → uint8 (H,W,3)."""
    im = Image.open(io.BytesIO(blob))
    if draft is not None:
        im.draft("RGB", draft)
    return np.asarray(im.convert("RGB"), dtype=np.uint8)


def segments(blob):
    """[(marker, offset of the marker's 0xFF, payload offset, payload length)] of every segment with a length, SOS
    headers of later scans included; the entropy-coded data behind an SOS is stepped over."""
    out, i, n = [], 2, len(blob)
    while i + 4 <= n:
        assert blob[i] == 0xFF, i
        m = blob[i + 1]
        if m == 0xFF:
            i += 1
            continue
        if m == 0xD9:
            break
        length = (blob[i + 2] << 8) | blob[i + 3]
        out.append((m, i, i + 4, length - 2))
        i += 2 + length
        if m == 0xDA:                                          # to the marker that closes the scan
            while i + 1 < n and not (blob[i] == 0xFF and blob[i + 1] not in (0x00, 0xFF) and not 0xD0 <= blob[i + 1] <= 0xD7):
                i += 1
    return out


def patch_hv(blob, hv):
    """The same file with the SOF's H/V byte of its one component set to `hv`."""
    b = bytearray(blob)
    (_, _, p, _), = [s for s in segments(blob) if s[0] in (0xC0, 0xC1, 0xC2)]
    assert b[p + 5] == 1 and b[p + 7] == 0x11
    b[p + 7] = hv
    return bytes(b)


def patch_id(blob, cid=PATCHED_ID):
    """The same file with its component called `cid` in the SOF and in every SOS."""
    b = bytearray(blob)
    for m, _, p, _ in segments(blob):
        if m in (0xC0, 0xC1, 0xC2):
            b[p + 6] = cid
        elif m == 0xDA:
            assert b[p] == 1
            b[p + 1] = cid
    return bytes(b)


def scan_range(blob):
    """(first, last + 1) entropy-coded byte of a baseline file's one scan."""
    m, _, p, n = segments(blob)[-1]
    assert m == 0xDA and blob[-2:] == b"\xff\xd9"
    return p + n, len(blob) - 2


def truncated(blob):
    """Cut in the middle of the scan: no EOI, too few intervals or MCUs that need bits past the end."""
    lo, hi = scan_range(blob)
    return blob[:(lo + hi) // 2]


def invalid_code(blob):
    """Eight entropy-coded bytes in the middle of the scan replaced by eight stuffed 0xFF bytes (byte-aligned, so the
    length stays): 64 one bits.  No Huffman code is all ones and the longest symbol takes 16 + 11 bits, so some symbol
    starts with at least 16 ones in front of it: an invalid code."""
    lo, hi = scan_range(blob)
    mid = (lo + hi) // 2
    assert hi - mid > 32
    return blob[:mid] + b"\xff\x00" * 8 + blob[mid + 16:]


def rst_out_of_sequence(blob):
    """The first RST0 of a file with restart markers renamed RST3."""
    lo, hi = scan_range(blob)
    at = blob.index(b"\xff\xd0", lo, hi)
    return blob[:at] + b"\xff\xd3" + blob[at + 2:]
