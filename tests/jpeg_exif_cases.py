"""JPEG files that carry an EXIF / XMP orientation: hand-made APP1 segments spliced into files from Pillow and from
tests/jpeg_writer.py.  Pillow's own writer only produces the plain form (one Exif APP1, SHORT, count 1), so every other
row of the table `jpeg.exif_orientation` has to agree with Pillow on is built here byte by byte.

`TAG_CASES`: name → (function blob → blob, the value Pillow's getexif() reports for 0x0112, the orientation
ImageOps.exif_transpose acts on).  The two last columns are what Pillow 12 does with the bytes; the host test checks
both against the installed Pillow before it holds the parser to them.
"""
import io
import struct

import numpy as np
from PIL import Image

import jpeg_writer as W
from jpeg_stream_cases import Q3
from test_jpeg_host import encode, smooth_rgb

BYTE, ASCII, SHORT, LONG = 1, 2, 3, 4
ORIENTATION, SOFTWARE = 0x0112, 0x0131
XMP_HEAD = b"http://ns.adobe.com/xap/1.0/\x00"


# ------------------------------------------------------------------------------------------------------------
# segments
# ------------------------------------------------------------------------------------------------------------
def entry(order, tag, typ, count, value: bytes):
    """One 12-byte IFD entry with an inline value (at most 4 bytes, zero padded)."""
    assert len(value) <= 4
    return struct.pack(order + "HHI", tag, typ, count) + value.ljust(4, b"\x00")


def number(order, typ, v):
    return struct.pack(order + {BYTE: "B", SHORT: "H", LONG: "I"}[typ], v)


def tiff(order, entries, mark=None):
    """TIFF header + IFD0 of the given entries + a zero next-IFD offset.  order: "<" (II) or ">" (MM)."""
    head = (mark or {"<": b"II", ">": b"MM"}[order]) + struct.pack(order + "HI", 42, 8)
    return head + struct.pack(order + "H", len(entries)) + b"".join(entries) + struct.pack(order + "I", 0)


def app1(payload: bytes):
    return b"\xff\xe1" + struct.pack(">H", len(payload) + 2) + payload


def exif_app1(tiff_bytes: bytes):
    return app1(b"Exif\x00\x00" + tiff_bytes)


def orientation_app1(value, order="<", typ=SHORT):
    """The plain form: one entry 0x0112, count 1."""
    return exif_app1(tiff(order, [entry(order, ORIENTATION, typ, 1, number(order, typ, value))]))


def xmp_app1(value, element=False):
    body = (f"<tiff:Orientation>{value}</tiff:Orientation>" if element else f'tiff:Orientation="{value}"').encode()
    packet = (b'<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
              b'<rdf:Description xmlns:tiff="http://ns.adobe.com/tiff/1.0/" ' +
              (b">" + body if element else body + b">") + b"</rdf:Description></rdf:RDF></x:xmpmeta>")
    return app1(XMP_HEAD + packet)


def splice(blob: bytes, segments: bytes, before_app0=False) -> bytes:
    """`segments` behind the JFIF APP0 that follows SOI (behind SOI itself if there is none, or with before_app0)."""
    assert blob[:2] == b"\xff\xd8"
    pos = 2
    if not before_app0 and blob[2:4] == b"\xff\xe0":
        pos = 4 + struct.unpack(">H", blob[4:6])[0]
    return blob[:pos] + segments + blob[pos:]


def with_orientation(blob: bytes, value: int, **kw) -> bytes:
    return splice(blob, orientation_app1(value, **kw))


# ------------------------------------------------------------------------------------------------------------
# the table of the issue: what Pillow reports, what it transposes by
# ------------------------------------------------------------------------------------------------------------
def _short2(order="<"):
    return exif_app1(tiff(order, [entry(order, ORIENTATION, SHORT, 2, number(order, SHORT, 6) + number(order, SHORT, 0))]))


def _truncated():
    whole = tiff("<", [entry("<", ORIENTATION, SHORT, 1, number("<", SHORT, 6))])
    return exif_app1(whole[:8 + 2 + 6])                                 # the header, the count, half an entry


def _no_tag():
    return exif_app1(tiff("<", [entry("<", SOFTWARE, ASCII, 3, b"ab\x00")]))


TAG_CASES = {
    "short_II_6": (lambda b: with_orientation(b, 6), 6, 6),
    "short_MM_6": (lambda b: with_orientation(b, 6, order=">"), 6, 6),
    "long_II_6": (lambda b: with_orientation(b, 6, typ=LONG), 6, 6),
    "long_MM_6": (lambda b: with_orientation(b, 6, order=">", typ=LONG), 6, 6),
    "ascii_6": (lambda b: splice(b, exif_app1(tiff("<", [entry("<", ORIENTATION, ASCII, 2, b"6\x00")]))), "6", 1),
    "byte_6": (lambda b: with_orientation(b, 6, typ=BYTE), b"\x06", 1),
    "value_0": (lambda b: with_orientation(b, 0), 0, 1),
    "value_9": (lambda b: with_orientation(b, 9), 9, 1),
    "short_count_2": (lambda b: splice(b, _short2()), 6, 6),
    "truncated_entry": (lambda b: splice(b, _truncated()), None, 1),
    "bad_byte_order": (lambda b: splice(b, exif_app1(tiff("<", [entry("<", ORIENTATION, SHORT, 1, b"\x06\x00")],
                                                          mark=b"XX"))), None, 1),
    "two_exif_6_then_3": (lambda b: splice(b, orientation_app1(6) + orientation_app1(3)), 6, 6),
    "xmp_attr_8": (lambda b: splice(b, xmp_app1(8)), 8, 8),
    "exif_1_xmp_8": (lambda b: splice(b, orientation_app1(1) + xmp_app1(8)), 1, 1),
    "exif_no_tag_xmp_element_5": (lambda b: splice(b, _no_tag() + xmp_app1(5, element=True)), 5, 5),
    "app1_before_app0": (lambda b: splice(b, orientation_app1(6), before_app0=True), 6, 6),
    "no_app1": (lambda b: b, None, 1),
}
for _o in range(1, 9):
    TAG_CASES[f"plain_{_o}"] = (lambda b, _o=_o: with_orientation(b, _o), _o, _o)


# ------------------------------------------------------------------------------------------------------------
# base files
# ------------------------------------------------------------------------------------------------------------
def gray(h, w, seed=0):
    return smooth_rgb(h, w, seed)[:, :, 1].copy()


def base_file(kind: str, size=(37, 23), seed=0) -> bytes:
    """One file of `size` (width, height) without any APP1: "444", "420_dri" (restart markers), "gray", "progressive",
    "gray_progressive" from Pillow, "writer" from tests/jpeg_writer.py (4:2:0, its own tables and header)."""
    w, h = size
    if kind == "444":
        return encode(smooth_rgb(h, w, seed), quality=90, subsampling=0)
    if kind == "420_dri":
        return encode(smooth_rgb(h, w, seed), quality=85, subsampling=2, restart_marker_blocks=2)
    if kind == "gray":
        return encode(gray(h, w, seed), quality=90)
    if kind == "progressive":
        return encode(smooth_rgb(h, w, seed), quality=90, subsampling=2, progressive=True)
    if kind == "gray_progressive":
        return encode(gray(h, w, seed), quality=90, progressive=True)
    if kind == "writer":
        coefs = W.coefficients_from_pixels(smooth_rgb(h, w, seed), 2, Q3)
        return W.write_jpeg(w, h, 2, coefs, Q3)[0]
    raise ValueError(kind)


KINDS = ("444", "420_dri", "gray", "progressive", "gray_progressive", "writer")


def pillow_tag(blob):
    with Image.open(io.BytesIO(blob)) as im:
        return im.getexif().get(ORIENTATION)
