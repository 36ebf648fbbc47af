"""Progressive JPEGs with per-component sampling on the device: four components (`cmyk="device"`) and three at any layout
(`layouts="all"`) with progressive="device", against `np.asarray(Image.open(f).convert("RGB"))` bit for bit; a mixed
batch with every other kind, the single opt-ins (host route), EXIF orientation, a draft request, the containment of
odic_jpeg_decode_progressive_any, and the records it refuses."""
import ctypes
import io
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import jpeg_cmyk_cases as K
import jpeg_layout_cases as L
import jpeg_prog_layout_cases as P
from guards import guarded
from jpeg_exif_cases import with_orientation
from jpeg_gray_cases import gray_file
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

EVERY = dict(non_rgb="convert", cmyk="device", layouts="all", progressive="device")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


@pytest.fixture(scope="module")
def oracles():
    """Pillow's pixels of every case file: computed once, never changed."""
    return {name: torch.from_numpy(P.oracle(c.blob).copy()) for name, c in P.CASES.items()}


@pytest.mark.parametrize("name", P.CASES)
def test_case_file(pre, oracles, name):
    """Each file in a call of its own, under exactly the two opt-ins its kind needs: the new route, status 0 (a fallen-back
    case has route "host-after-status" and fails here), Pillow's pixels."""
    c = P.CASES[name]
    kw = dict(progressive="device", **P.KW[c.ncomp])
    got, = pre.decode_jpeg([c.blob], **kw)
    assert pre.last_routes == (c.route,)
    assert got.shape == oracles[name].shape and torch.equal(got.cpu(), oracles[name])


def test_all_cases_as_one_batch_never_ask_pillow(pre, oracles, monkeypatch):
    """No silent host fallback: with the PIL decode taken away the whole case list decodes, in one batch."""
    def boom(*a, **k):
        raise AssertionError("host decode")
    monkeypatch.setattr(pre, "_host_rgb", boom)
    names = list(P.CASES)
    random.Random(3).shuffle(names)
    got = pre.decode_jpeg([P.CASES[n].blob for n in names], **EVERY)
    assert list(pre.last_routes) == [P.CASES[n].route for n in names]
    wrong = [n for n, g in zip(names, got) if g.shape != oracles[n].shape or not torch.equal(g.cpu(), oracles[n])]
    assert not wrong, wrong


def mixed():
    """(file, route with every opt-in) of one shuffled batch of every kind."""
    files = [(encode(smooth_rgb(48, 64, seed=1), quality=90, subsampling=2), "device"),
             (encode(smooth_rgb(40, 56, seed=2), quality=90, subsampling=1, progressive=True), "device-progressive"),
             (gray_file("dri3", (37, 53)), "device"),
             (K.CASES["cmyk-sub2-48x64"][0], "device-cmyk"),
             (L.CASES["440-17x33"].blob, "device-layout"),
             (P.CASES["440-17x33"].blob, "device-progressive-layout"),
             (P.CASES["410-dri3"].blob, "device-progressive-layout"),
             (P.CASES["rgb-bare-7x9"].blob, "device-progressive-layout"),
             (P.CASES["photoshop-48x64"].blob, "device-progressive-cmyk"),
             (P.CASES["pillow-cmyk-sub2-17x33"].blob, "device-progressive-cmyk"),
             (P.CASES["c4-21-partial-dc"].blob, "device-progressive-cmyk")]
    random.Random(11).shuffle(files)
    return [f for f, _ in files], [r for _, r in files]


def test_mixed_batch_and_the_single_opt_ins(pre):
    blobs, routes = mixed()
    want = [torch.from_numpy(P.oracle(b).copy()) for b in blobs]
    got = pre.decode_jpeg(blobs, **EVERY)
    assert list(pre.last_routes) == routes
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g.cpu(), w), k
    # one opt-in alone leaves the new kinds with PIL: identical pixels, and the other kinds keep the route they had
    new = {"device-progressive-cmyk", "device-progressive-layout"}
    for kw, lost in ((dict(progressive="device"), new | {"device-cmyk", "device-layout"}),
                     (dict(cmyk="device"), new | {"device-progressive", "device-layout"}),
                     (dict(layouts="all"), new | {"device-progressive", "device-cmyk"}),
                     (dict(cmyk="device", layouts="all"), new | {"device-progressive"})):
        plain = pre.decode_jpeg(blobs, non_rgb="convert", **kw)
        assert list(pre.last_routes) == ["host" if r in lost else r for r in routes], kw
        assert all(torch.equal(g, h) for g, h in zip(got, plain)), kw
    # progressive="device" with the opt-in of the OTHER kind: each new kind needs its own
    pre.decode_jpeg(blobs, non_rgb="convert", progressive="device", cmyk="device")
    assert [r for r in pre.last_routes if r in new] == ["device-progressive-cmyk"] * 3
    pre.decode_jpeg(blobs, non_rgb="convert", progressive="device", layouts="all")
    assert [r for r in pre.last_routes if r in new] == ["device-progressive-layout"] * 3
    host = pre.from_jpeg_bytes(blobs, non_rgb="convert")
    assert torch.equal(pre.from_jpeg_bytes(blobs, **EVERY), host)
    regions = [(routes.index("device-progressive-layout"), (1.5, 2.0, 6.0, 8.25)),
               (routes.index("device-progressive-cmyk"), (0.0, 1.0, 7.0, 8.5))]
    assert torch.equal(pre.from_jpeg_bytes(blobs, regions=regions, **EVERY),
                       pre.from_jpeg_bytes(blobs, regions=regions, non_rgb="convert"))


def test_orientation_tag_6_on_progressive_440(pre):
    blob = with_orientation(P.CASES["440-17x33"].blob, 6)
    want = np.asarray(Image.fromarray(P.oracle(blob)).transpose(Image.Transpose.ROTATE_270))    # what tag 6 asks for
    assert np.array_equal(want, np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB")))
    got, = pre.decode_jpeg([blob], orientation="exif", **EVERY)
    assert pre.last_routes == ("device-progressive-layout",) and pre.last_orientations == (6,)
    assert want.shape == (17, 33, 3) and np.array_equal(got.cpu().numpy(), want)


def test_draft_request_keeps_them_on_the_host(pre):
    blobs = [P.CASES["440-48x64"].blob, P.CASES["photoshop-48x64"].blob]
    got = pre.decode_jpeg(blobs, draft=(8, 8), **EVERY)
    assert list(pre.last_routes) == ["host", "host"]
    for g, b in zip(got, blobs):
        im = Image.open(io.BytesIO(b))
        im.draft("RGB", (8, 8))
        assert np.array_equal(g.cpu().numpy(), np.asarray(im.convert("RGB")))


# ------------------------------------------------------------------------------------------------------------
# through the C ABI, the parser's word taken for granted or bypassed: containment, and the records the kernels refuse
# ------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


def run_record(pre, hd, blob, edit=None):
    """One odic_jpeg_decode_progressive_any call on the header `hd` of `blob`, every device buffer exactly as large as
    asked for inside a poisoned allocation (guards.py).  edit(rec, srec): changes the packed records first.
    → (status, the image's output bytes, the guarded buffers)."""
    from on_device_image_captioning_amd import _hip
    lib = _hip.load()
    rec, srec, trec, tot, out_offs, out_bytes = J.pack_progressive([hd], [0], dtype=J.PROG_HEADER_ANY_DTYPE)
    if edit is not None:
        edit(rec, srec)
    batch = _hip.JpegProgBatch()
    batch.n_images = 1
    pre._set_fields(batch, tot)
    need = lib.odic_jpeg_progressive_any_workspace_bytes(ctypes.byref(batch))
    assert need > 0
    dev = "cuda:0"
    put = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev)
    drec, dsrec, dtrec, data = put(rec), put(srec), put(trec), put(np.frombuffer(blob, np.uint8))
    ws = guarded(1, need, need, torch.uint8, dev)
    out = guarded(1, out_bytes, out_bytes, torch.uint8, dev)
    out.t.fill_(SENTINEL)
    status = guarded(1, 1, 1, torch.int32, dev)
    batch.headers, batch.scans, batch.tables = drec.data_ptr(), dsrec.data_ptr(), dtrec.data_ptr()
    batch.data, batch.out, batch.status = data.data_ptr(), out.data_ptr(), status.data_ptr()
    _hip.check(lib.odic_jpeg_decode_progressive_any(ctypes.byref(batch), ws.data_ptr(), need,
                                                    torch.cuda.current_stream().cuda_stream),
               "odic_jpeg_decode_progressive_any")
    torch.cuda.synchronize()
    return int(status.t.view(-1)[0]), out.t.view(-1).cpu().numpy(), (ws, out, status)


@pytest.mark.parametrize("name", ["410-17x33", "photoshop-17x33"])
def test_progressive_any_decode_stays_inside_its_workspace(pre, name):
    c = P.CASES[name]
    hd = J.parse_progressive(c.blob, **P.KW[c.ncomp])
    st, px, bufs = run_record(pre, hd, c.blob)
    assert st == 0 and np.array_equal(px.reshape(33, 17, 3), P.oracle(c.blob))
    for g in bufs:
        g.assert_untouched(what=f"{name}: {g.dtype} buffer of {g.cols} elements")


def factor_of_five(rec, srec):
    rec["h"][0, 0] = 5


def mask_names_component_3(rec, srec):
    srec["comp_mask"][-1] = 8


@pytest.mark.parametrize("edit", [factor_of_five, mask_names_component_3])
def test_refused_records_write_nothing(pre, edit):
    """A record that breaks the frame rules, and a scan that names a component the frame lacks: status 1, the image's
    output bytes keep their sentinel, nothing outside the buffers is touched."""
    c = P.CASES["440-17x33"]
    hd = J.parse_progressive(c.blob, **P.KW[3])
    st, px, bufs = run_record(pre, hd, c.blob, edit)
    assert st == 1 and (px == SENTINEL).all()
    for g in bufs:
        g.assert_untouched(what=edit.__name__)


def test_scan_cut_short_by_a_marker_writes_nothing(pre):
    """The last AC scan ends early at a marker placed mid-scan.  The parser turns the file away; here its records come
    from the whole file's header, with the last scan's range set to the cut data and the marker behind it."""
    c = P.cut_short()
    assert J.parse_progressive(c.blob, **P.KW[3]).kind == J.HOST
    whole = P.Case("410", 17, 33, 7)
    hd = J.parse_progressive(whole.blob, **P.KW[3])
    assert hd.kind == J.DEVICE and c.blob[:hd.scans[-1].data_offset] == whole.blob[:hd.scans[-1].data_offset]
    hd.scans[-1].data_end = len(c.blob) - 2                      # up to the EOI: the marker lies inside the range
    assert c.blob[hd.scans[-1].data_end - 2:hd.scans[-1].data_end] == b"\xff\xdc"
    st, px, bufs = run_record(pre, hd, c.blob)
    assert st == 1 and (px == SENTINEL).all()
    for g in bufs:
        g.assert_untouched(what="cut scan")
    st, px, _ = run_record(pre, J.parse_progressive(whole.blob, **P.KW[3]), whole.blob)       # the whole file decodes
    assert st == 0 and np.array_equal(px.reshape(33, 17, 3), P.oracle(whole.blob))
