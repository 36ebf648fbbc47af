"""CPU side of the device JPEG decoder: the host marker parser against Pillow, the sorting of
files into device / black / host kinds, a numpy model of the device arithmetic (Huffman with the device lookup
tables, DC prediction, ISLOW IDCT with libjpeg's masked range limit, fancy upsampling, fixed-point YCbCr→RGB)
checked bit for bit against `np.asarray(Image.open(f))`, and the argument checks of the C entry points."""
import ctypes
import io
import os

import numpy as np
import pytest
from PIL import Image, JpegImagePlugin

from on_device_image_captioning_amd import jpeg as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "tests", "golden", "demo_material")


def smooth_rgb(h, w, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / (7 + seed) + y / 13), 128 + 90 * np.cos(y / (5 + seed) - x / 17),
                    128 + 60 * np.sin((x + y) / 9)], axis=2)
    img += rng.normal(0, 12, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


# the parser matrix: (size (w, h), save kwargs)
MATRIX = [((40, 24), dict(subsampling=s, quality=q)) for s in (0, 1, 2) for q in (50, 90, 100)] + [
    ((48, 40), dict(subsampling=2, quality=90, optimize=True)),
    ((48, 40), dict(subsampling=1, quality=75, optimize=True)),
    ((56, 40), dict(subsampling=2, quality=90, restart_marker_blocks=3)),
    ((56, 40), dict(subsampling=0, quality=90, restart_marker_rows=1)),
    ((1, 1), dict(subsampling=2, quality=90)),
    ((17, 9), dict(subsampling=2, quality=90)),
    ((17, 9), dict(subsampling=1, quality=95)),
    ((31, 2000), dict(subsampling=2, quality=90)),
]


def flat_dqt(blob, value=255):
    """`blob` with every quantisation table entry replaced by `value`: a legal baseline file whose dequantised
    coefficients leave the range where libjpeg-turbo's SIMD and C IDCTs agree (for noise encoded at quality 100)."""
    b = bytearray(blob)
    i = 2
    while b[i + 1] != 0xDA:
        seg = (b[i + 2] << 8) | b[i + 3]
        if b[i + 1] == 0xDB:
            j = i + 4
            while j < i + 2 + seg:
                wide = b[j] >> 4
                for k in range(64):
                    if wide:
                        b[j + 1 + 2 * k], b[j + 2 + 2 * k] = value >> 8, value & 255
                    else:
                        b[j + 1 + k] = value
                j += 1 + 64 * (wide + 1)
        i += 2 + seg
    return bytes(b)


def out_of_range_blob():
    noise = np.random.default_rng(0).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    return flat_dqt(encode(noise, quality=100, subsampling=0))


def matrix_blobs():
    return [encode(smooth_rgb(h, w, seed=k % 5), **kw) for k, ((w, h), kw) in enumerate(MATRIX)]


@pytest.mark.parametrize("k", range(len(MATRIX)))
def test_parser_agrees_with_pillow(k):
    (w, h), kw = MATRIX[k]
    blob = encode(smooth_rgb(h, w, seed=k % 5), **kw)
    hd = J.parse(blob)
    im = Image.open(io.BytesIO(blob))
    assert hd.kind == J.DEVICE, hd.reason
    assert (hd.width, hd.height) == im.size
    samp = JpegImagePlugin.get_sampling(im)
    assert hd.sampling == {0: 0, 1: 1, 2: 2}[samp]
    for c in range(3):                                    # both in natural (row-major) order
        tq = im.layer[c][3]
        assert list(hd.qtables[c]) == list(im.quantization[tq])
    if "restart_marker_blocks" in kw or "restart_marker_rows" in kw:
        assert hd.restart_interval > 0
    else:
        assert hd.restart_interval == 0


def test_kinds():
    tatin = open(os.path.join(DEMO, "tatin.jpg"), "rb").read()
    micheal = open(os.path.join(DEMO, "micheal.jpg"), "rb").read()
    assert J.parse(tatin).kind == J.HOST                          # progressive
    assert J.parse(micheal).kind == J.DEVICE
    png = io.BytesIO()
    Image.fromarray(smooth_rgb(8, 8)).save(png, format="PNG")
    assert J.parse(png.getvalue()).kind == J.HOST
    assert J.parse(micheal[:300]).kind == J.HOST                  # header cut short
    assert J.parse(b"").kind == J.HOST
    g = io.BytesIO()
    Image.fromarray(smooth_rgb(8, 8)[:, :, 0]).save(g, format="JPEG")
    hd = J.parse(g.getvalue())
    assert hd.kind == J.BLACK and (hd.width, hd.height) == (8, 8)
    c = io.BytesIO()
    Image.fromarray(smooth_rgb(8, 8)).convert("CMYK").save(c, format="JPEG")
    assert J.parse(c.getvalue()).kind == J.BLACK
    p = io.BytesIO()
    Image.fromarray(smooth_rgb(16, 16)).save(p, format="JPEG", progressive=True)
    assert J.parse(p.getvalue()).kind == J.HOST


def random_rgb():
    """The 24x40 image of the prefix sweeps (here and in test_jpeg_progressive_host.py)."""
    return np.random.default_rng(7).integers(0, 256, (40, 24, 3), dtype=np.uint8)


def header_fields(hd):
    """Every field of a header but `reason`, in a form that compares with == (tables as lists / bytes)."""
    return [(f, [list(map(int, q)) for q in v] if f == "qtables" else
             [(t.bits, bytes(t.vals)) for t in v] if f in ("dc_tables", "ac_tables") else v)
            for f, v in vars(hd).items() if f != "reason"]


@pytest.mark.parametrize("kw", [dict(subsampling=2), dict(subsampling=0, restart_marker_blocks=2)], ids=["420", "444-dri"])
def test_every_prefix_of_a_baseline_file_is_sorted_without_raising(kw):
    """Neither parser raises on any prefix; `parse` needs the whole header and one byte of scan data, and from
    there on returns the full file's header (it never looks at the entropy-coded data)."""
    blob = encode(random_rgb(), quality=50, **kw)
    full = J.parse(blob)
    assert full.kind == J.DEVICE and (full.restart_interval > 0) == ("restart_marker_blocks" in kw)
    want = header_fields(full)
    for n in range(len(blob)):
        hd = J.parse(blob[:n])
        assert J.parse_progressive(blob[:n]).kind == J.HOST, n                # SOF0, or cut before it
        if n <= full.data_offset:
            assert hd.kind == J.HOST and hd.reason, n
        else:
            assert header_fields(hd) == want, n


def test_device_tables_decode_every_code():
    hd = J.parse(encode(smooth_rgb(24, 24), quality=90, optimize=True))
    for t in hd.dc_tables + hd.ac_tables:
        lut, maxcode, valoff, huffval = J.device_tables(t)
        code, p = 0, 0
        for length in range(1, 17):
            for _ in range(t.bits[length - 1]):
                peek = code << (16 - length)
                assert _lookup(lut, maxcode, valoff, huffval, peek) == (length, t.vals[p])
                code += 1
                p += 1
            code <<= 1


# ------------------------------------------------------------------------------------------------------------
# numpy model of csrc/jpeg_decode.hip
# ------------------------------------------------------------------------------------------------------------
def _lookup(lut, maxcode, valoff, huffval, peek16):
    e = int(lut[peek16 >> (16 - J.LUT_BITS)])
    if e:
        return e >> 8, e & 255
    for length in range(J.LUT_BITS + 1, 17):
        code = peek16 >> (16 - length)
        if code <= maxcode[length]:
            return length, int(huffval[code + valoff[length]])
    return None


def _intervals(blob, start):
    """Destuffed entropy data split at the restart markers (what the device's segment kernel produces)."""
    segs, cur, i = [], bytearray(), start
    while True:
        b = blob[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        m = blob[i + 1]
        if m == 0:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            assert m - 0xD0 == len(segs) % 8
            segs.append(bytes(cur))
            cur = bytearray()
        elif m == 0xD9:
            segs.append(bytes(cur))
            return segs
        else:
            raise AssertionError(f"marker {m:02X}")
        i += 2


def model_coefficients(blob, hd):
    """Huffman decode with the device tables → int16 [blocks, 64] natural order, DC as a difference."""
    tabs = [J.device_tables(t) for t in hd.dc_tables + hd.ac_tables]
    nY = (1, 2, 4)[hd.sampling]
    comp = [0] * nY + [1, 2]
    bpm = len(comp)
    nmcu = hd.mcus_x * hd.mcus_y
    R = hd.restart_interval or nmcu
    coef = np.zeros((nmcu * bpm, 64), np.int16)
    segs = _intervals(blob, hd.data_offset)
    assert len(segs) == -(-nmcu // R)
    b = 0
    for seg in segs:
        bits = int.from_bytes(seg + b"\xff" * 8, "big")
        nbits = (len(seg) + 8) * 8
        pos = 0

        def peek(n):
            return (bits >> (nbits - pos - n)) & ((1 << n) - 1)

        for _ in range(min(R, nmcu - b // bpm) * bpm):
            c = comp[b % bpm]
            ln, s = _lookup(*tabs[c], peek(16))
            pos += ln
            v = peek(s) if s else 0
            pos += s
            if s and v < (1 << (s - 1)):
                v -= (1 << s) - 1
            coef[b, 0] = v
            k = 1
            while k < 64:
                ln, rs = _lookup(*tabs[3 + c], peek(16))
                pos += ln
                r, s = rs >> 4, rs & 15
                if s:
                    k += r
                    v = peek(s)
                    pos += s
                    if v < (1 << (s - 1)):
                        v -= (1 << s) - 1
                    coef[b, J.NATURAL_ORDER[k]] = v
                elif r != 15:
                    break
                else:
                    k += 15
                k += 1
            b += 1
        assert pos <= len(seg) * 8
    return coef


class Rejected(Exception):
    """The device sets kErrRange: the values leave the range where libjpeg-turbo's SIMD and C IDCTs agree."""


IDCT_LIMIT = 8191                                         # kIdctLimit of csrc/jpeg_decode.hip


def model_dc_prediction(coef, hd):
    nY = (1, 2, 4)[hd.sampling]
    comp = np.array([0] * nY + [1, 2])
    bpm = len(comp)
    nmcu = hd.mcus_x * hd.mcus_y
    R = hd.restart_interval or nmcu
    c = coef.astype(np.int64).reshape(nmcu, bpm, 64)
    out = c.copy()
    for start in range(0, nmcu, R):
        for ci in range(3):
            cols = np.nonzero(comp == ci)[0]
            d = c[start:start + R][:, cols, 0].reshape(-1)
            out[start:start + R, cols, 0] = np.cumsum(d).reshape(-1, len(cols))
    if out[:, :, 0].min() < -32768 or out[:, :, 0].max() > 32767:     # JCOEF would wrap
        raise Rejected("DC")
    return out.reshape(-1, 64).astype(np.int16)          # JCOEF is a short


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def model_idct(blocks, q):
    """jidctint.c jpeg_idct_islow on [n, 64] dequantised with q[64] → uint8 [n, 8, 8]."""
    F = dict(c0298=2446, c0390=3196, c0541=4433, c0765=6270, c0899=7373, c1175=9633, c1501=12299, c1847=15137,
             c1961=16069, c2053=16819, c2562=20995, c3072=25172)

    def one_d(v, shift):                                  # v: [..., 8] along the transformed axis
        z2, z3 = v[..., 2], v[..., 6]
        z1 = (z2 + z3) * F["c0541"]
        tmp2 = z1 - z3 * F["c1847"]
        tmp3 = z1 + z2 * F["c0765"]
        tmp0 = (v[..., 0] + v[..., 4]) << 13
        tmp1 = (v[..., 0] - v[..., 4]) << 13
        t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * F["c1175"]
        t0, t1, t2, t3 = t0 * F["c0298"], t1 * F["c2053"], t2 * F["c3072"], t3 * F["c1501"]
        z1, z2, z3, z4 = z1 * -F["c0899"], z2 * -F["c2562"], z3 * -F["c1961"] + z5, z4 * -F["c0390"] + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        o = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
        return np.stack([_descale(x, shift) for x in o], axis=-1)

    d = blocks.astype(np.int64).reshape(-1, 8, 8) * q.astype(np.int64).reshape(1, 8, 8)
    ws = one_d(np.swapaxes(d, 1, 2), 13 - 2)              # columns: [n, col, row]
    ws = np.swapaxes(ws, 1, 2)                            # [n, row, col]
    x = one_d(ws, 13 + 2 + 3)
    if np.abs(d).max(initial=0) > IDCT_LIMIT or np.abs(ws).max(initial=0) > IDCT_LIMIT or \
            x.min(initial=0) < -512 or x.max(initial=0) > 511:
        raise Rejected("IDCT range")
    s = ((x + 512) & 1023) - 512                          # range_limit[x & RANGE_MASK] of the post-IDCT table
    return np.clip(s + 128, 0, 255).astype(np.uint8)


def model_planes(blob, hd):
    coef = model_dc_prediction(model_coefficients(blob, hd), hd)
    hy, vy = hd.comp_hv[0]
    nY = hy * vy
    bpm = nY + 2
    mx, my = hd.mcus_x, hd.mcus_y
    planes = [np.zeros((my * 8 * vy, mx * 8 * hy), np.uint8), np.zeros((my * 8, mx * 8), np.uint8),
              np.zeros((my * 8, mx * 8), np.uint8)]
    pix = [model_idct(coef.reshape(-1, bpm, 64)[:, j], hd.qtables[0 if j < nY else j - nY + 1]) for j in range(bpm)]
    for j in range(bpm):
        c = 0 if j < nY else j - nY + 1
        bx, by = (j % hy, j // hy) if c == 0 else (0, 0)
        hh, vv = (hy, vy) if c == 0 else (1, 1)
        p = pix[j].reshape(my, mx, 8, 8)
        for yy in range(my):
            for xx in range(mx):
                r0, c0 = (yy * vv + by) * 8, (xx * hh + bx) * 8
                planes[c][r0:r0 + 8, c0:c0 + 8] = p[yy, xx]
    return planes


def model_rgb(blob):
    hd = J.parse(blob)
    assert hd.kind == J.DEVICE
    Yp, Cb, Cr = model_planes(blob, hd)
    W, H = hd.width, hd.height
    hy, vy = hd.comp_hv[0]
    dw, dh = -(-W // hy), -(-H // vy)
    x, y = np.arange(W), np.arange(H)
    Y = Yp[:H, :W].astype(np.int64)

    def up(P):
        P = P.astype(np.int64)
        if hy == 1:
            return P[:H, :W]
        c = x >> 1
        if dw <= 2:                                       # jdsample.c: a component at most two samples wide is
            return P[(y >> 1) if vy == 2 else y][:, c]    # replicated (h2v1_upsample / h2v2_upsample), not filtered
        cn = np.where(x & 1, np.minimum(c + 1, dw - 1), np.maximum(c - 1, 0))
        if vy == 1:                                       # h2v1_fancy_upsample
            a, b = P[:H][:, c], P[:H][:, cn]
            return np.where(x & 1, (3 * a + b + 2) >> 2, (3 * a + b + 1) >> 2)
        r = y >> 1                                        # h2v2_fancy_upsample
        rn = np.where(y & 1, np.minimum(r + 1, dh - 1), np.maximum(r - 1, 0))
        cs = 3 * P[r] + P[rn]                             # column sums [H, dw+...]
        a, b = cs[:, c], cs[:, cn]
        return np.where(x & 1, (3 * a + b + 7) >> 4, (3 * a + b + 8) >> 4)

    cb, cr = up(Cb) - 128, up(Cr) - 128

    def fix(v):
        return int(v * 65536 + 0.5)
    r = Y + ((fix(1.40200) * cr + 32768) >> 16)
    g = Y + ((-fix(0.34414) * cb + 32768 - fix(0.71414) * cr) >> 16)
    b = Y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("k", [k for k, ((w, h), _) in enumerate(MATRIX) if w * h <= 20000])   # Python Huffman: small only
def test_numpy_model_is_bit_exact_with_pillow(k):
    (w, h), kw = MATRIX[k]
    blob = encode(smooth_rgb(h, w, seed=k % 5), **kw)
    want = np.asarray(Image.open(io.BytesIO(blob)))
    got = model_rgb(blob)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.abs(got.astype(int) - want).max()


def test_numpy_model_on_a_photo_crop():
    src = Image.open(os.path.join(DEMO, "micheal.jpg")).convert("RGB")
    for k, samp in enumerate((0, 1, 2)):
        crop = np.asarray(src.crop((100 + 37 * k, 80, 100 + 37 * k + 53, 80 + 35)))
        blob = encode(crop, quality=90, subsampling=samp)
        assert np.array_equal(model_rgb(blob), np.asarray(Image.open(io.BytesIO(blob))))


def test_coefficients_outside_the_simd_range_are_rejected():
    """A legal baseline file (flat DQT of 255 over quality-100 noise: |coef·q| up to 42330) whose pixels differ between
    libjpeg-turbo's 16-bit SIMD IDCT (what Pillow runs) and the exact arithmetic: the model, like the device, rejects it
    so that the caller decodes it with PIL."""
    blob = out_of_range_blob()
    assert J.parse(blob).kind == J.DEVICE
    with pytest.raises(Rejected):
        model_rgb(blob)


def test_extreme_legitimate_images_stay_in_range():
    """1-pixel checkerboards and binary noise at quality 100 are the largest coefficients an encoder of 8-bit images
    produces; they must decode on the device, bit-exact."""
    cb = ((np.indices((32, 32)).sum(0) % 2) * 255).astype(np.uint8)
    bn = (np.random.default_rng(2).integers(0, 2, (32, 32, 3)) * 255).astype(np.uint8)
    for img, samp in ((np.stack([cb] * 3, 2), 0), (np.stack([cb, 255 - cb, cb], 2), 0), (bn, 0), (bn, 2)):
        blob = encode(img, quality=100, subsampling=samp)
        assert np.array_equal(model_rgb(blob), np.asarray(Image.open(io.BytesIO(blob))))


def test_scan_longer_than_the_device_limit_goes_to_the_host():
    blob = encode(smooth_rgb(16, 16), quality=90)
    hd = J.parse(blob)
    n = hd.data_offset + J.MAX_SCAN_BYTES + 1 - len(blob)
    big = blob[:-2] + bytes(n) + blob[-2:]                # extraneous bytes before EOI
    assert J.parse(big).kind == J.HOST


# ------------------------------------------------------------------------------------------------------------
# C entry points: rejected arguments need no GPU
# ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from on_device_image_captioning_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load()


def test_c_entry_points_reject_bad_arguments(lib):
    assert lib.odic_jpeg_decode(None, None, 0, None) == -2
    from on_device_image_captioning_amd import _hip
    b = _hip.JpegBatch()
    assert lib.odic_jpeg_decode(ctypes.byref(b), None, 0, None) == -2          # NULL headers / data / out / status
    b.headers, b.data, b.out, b.status = 16, 16, 16, 16
    b.n_images, b.subseq_bits, b.max_sync_passes = 1, 512, 4
    b.max_units = b.max_intervals = b.max_width = b.max_height = 1
    b.max_blocks = b.max_scan_bytes = b.total_scan_bytes = b.total_intervals = b.total_units = 1
    b.total_blocks = b.total_plane_bytes = 1
    need = lib.odic_jpeg_workspace_bytes(ctypes.byref(b))
    assert need > 0
    assert lib.odic_jpeg_decode(ctypes.byref(b), None, need, None) == -2         # no workspace
    assert lib.odic_jpeg_decode(ctypes.byref(b), 16, need - 1, None) == -1       # workspace too small
    for field, bad in (("n_images", 0), ("subseq_bits", 16), ("max_sync_passes", -1), ("max_sync_passes", 1000),
                       ("max_units", 0)):
        old = getattr(b, field)
        setattr(b, field, bad)
        assert lib.odic_jpeg_decode(ctypes.byref(b), 16, need, None) == -1, field
        setattr(b, field, old)
    assert lib.odic_jpeg_workspace_bytes(None) == 0


def test_header_record_matches_the_c_struct():
    assert J.HEADER_DTYPE.itemsize == 9016                    # sizeof(odic_jpeg_header), static_assert in the HIP
    assert J.HEADER_DTYPE.fields["qt"][1] == 88 and J.HEADER_DTYPE.fields["huffval"][1] == 7480
