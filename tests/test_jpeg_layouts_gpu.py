"""Three-component JPEGs at every baseline sampling layout on the device: `decode_jpeg(..., layouts="all")` against
`np.asarray(Image.open(f).convert("RGB"))` bit for bit under four knob settings, a mixed batch with every other kind, the
default's routes, a draft request, EXIF orientation, and the containment of odic_jpeg_any_decode; then that entry point
through the C ABI: one call that holds three- and four-component files, its containment, and the records it refuses."""
import ctypes
import io
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageOps

import jpeg_cmyk_cases as K
import jpeg_layout_cases as L
from guards import POISON, guarded
from jpeg_exif_cases import with_orientation
from jpeg_gray_cases import gray_file
from jpeg_layout_writer import write_jpeg3
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

KNOBS = {"default": dict(), "subseq32": dict(subseq_bits=32), "serial": dict(max_sync_passes=0),
         "subseq32-serial": dict(subseq_bits=32, max_sync_passes=0)}
ALL = dict(layouts="all")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


@pytest.fixture(scope="module")
def oracles():
    return {name: torch.from_numpy(L.oracle(c.blob).copy()) for name, c in L.CASES.items()}


@pytest.mark.parametrize("knobs", KNOBS)
def test_every_case_file(pre, oracles, knobs):
    names = list(L.CASES)
    got = pre.decode_jpeg([L.CASES[n].blob for n in names], **ALL, **KNOBS[knobs])
    routes = dict(zip(names, pre.last_routes))
    assert routes == {n: "device-layout" for n in names}         # none on the host, none "host-after-status"
    wrong = [n for n, g in zip(names, got) if g.shape != oracles[n].shape or not torch.equal(g.cpu(), oracles[n])]
    assert not wrong, wrong
    for n in names[::11]:                                        # ... and alone
        g, = pre.decode_jpeg([L.CASES[n].blob], **ALL, **KNOBS[knobs])
        assert pre.last_routes == ("device-layout",) and torch.equal(g.cpu(), oracles[n]), n


def mixed():
    files = [(encode(smooth_rgb(48, 64, seed=1), quality=90, subsampling=2), "device", "device"),
             (encode(smooth_rgb(40, 56, seed=2), quality=90, subsampling=1, progressive=True), "device-progressive",
              "device-progressive"),
             (gray_file("dri3", (37, 53)), "device", "device"),
             (K.CASES["cmyk-sub2-48x64"][0], "device-cmyk", "device-cmyk"),
             (L.CASES["440-17x33"].blob, "device-layout", "host"),
             (L.CASES["411-dri3"].blob, "device-layout", "host"),
             (L.CASES["410-48x64"].blob, "device-layout", "host"),
             (L.CASES["rgb-22-17x33"].blob, "device-layout", "host"),
             (L.CASES["11-21-21-7x9"].blob, "device-layout", "host")]
    random.Random(7).shuffle(files)
    return [f for f, _, _ in files], [r for _, r, _ in files], [r for _, _, r in files]


def test_mixed_batch_and_the_default(pre):
    blobs, routes, default_routes = mixed()
    want = [torch.from_numpy(L.oracle(b).copy()) for b in blobs]
    kw = dict(non_rgb="convert", cmyk="device", progressive="device")
    got = pre.decode_jpeg(blobs, **kw, **ALL)
    assert list(pre.last_routes) == routes
    plain = pre.decode_jpeg(blobs, **kw)                         # without the keyword: the same pixels, by PIL
    assert list(pre.last_routes) == default_routes
    for k, (g, h, w) in enumerate(zip(got, plain, want)):
        assert torch.equal(g.cpu(), w) and torch.equal(g, h), k
    assert torch.equal(pre.from_jpeg_bytes(blobs, **kw, **ALL), pre.from_jpeg_bytes(blobs, **kw))
    regions = [(routes.index("device-layout"), (1.5, 2.0, 6.0, 8.25)), (0, (0.0, 1.0, 7.0, 8.5))]
    assert torch.equal(pre.from_jpeg_bytes(blobs, regions=regions, **kw, **ALL),
                       pre.from_jpeg_bytes(blobs, regions=regions, **kw))
    with pytest.raises(ValueError, match="layouts"):
        pre.decode_jpeg(blobs, layouts="every")


def test_draft_request_and_refused_files_stay_on_the_host(pre):
    blobs = [L.CASES["440-48x64"].blob, L.CASES["411-48x64"].blob]
    got = pre.decode_jpeg(blobs, draft=(8, 8), **ALL)
    assert list(pre.last_routes) == ["host", "host"]
    for g, b in zip(got, blobs):
        im = Image.open(io.BytesIO(b))
        im.draft("RGB", (8, 8))
        assert np.array_equal(g.cpu().numpy(), np.asarray(im.convert("RGB")))
    f = L.refused()["Adobe transform 2"][0]
    g, = pre.decode_jpeg([f], **ALL)
    assert pre.last_routes == ("host",) and np.array_equal(g.cpu().numpy(), L.oracle(f))


def test_orientation_tag_6(pre):
    blob = with_orientation(L.CASES["440-17x33"].blob, 6)
    want = np.asarray(Image.fromarray(L.oracle(blob)).transpose(Image.Transpose.ROTATE_270))    # what tag 6 asks for
    assert np.array_equal(want, np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(blob))).convert("RGB")))
    got, = pre.decode_jpeg([blob], orientation="exif", **ALL)
    assert pre.last_routes == ("device-layout",) and pre.last_orientations == (6,)
    assert want.shape == (17, 33, 3) and np.array_equal(got.cpu().numpy(), want)


def guarded_preprocessor(monkeypatch):
    """A DevicePreprocessor whose workspace, compressed-data copy, RGB output and `status` are each exactly as large as
    asked for inside a poisoned allocation → (it, the list the guarded buffers are appended to)."""
    from on_device_image_captioning_amd import image_utils
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    made = []
    orig = DevicePreprocessor._grow

    def exact(buf, nbytes, **kw):
        if "device" not in kw:
            return orig(buf, nbytes, **kw)
        g = guarded(1, max(nbytes, 1), max(nbytes, 1), torch.uint8, kw["device"])
        made.append(g)
        return g.t.view(-1)

    class TorchWithGuardedEmpty:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*size, **kw):
            if kw.get("device") is not None and not kw.get("pin_memory") and len(size) == 1 and isinstance(size[0], int) \
                    and kw.get("dtype") in (torch.uint8, torch.int32) and torch.device(kw["device"]).type == "cuda":
                g = guarded(1, size[0], size[0], kw["dtype"], kw["device"])
                made.append(g)
                return g.t.view(-1)
            return torch.empty(*size, **kw)

    monkeypatch.setattr(DevicePreprocessor, "_grow", staticmethod(exact))
    fresh = DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)
    monkeypatch.setattr(image_utils, "torch", TorchWithGuardedEmpty())
    return fresh, made


def test_layout_decode_stays_inside_its_workspace(pre, monkeypatch):
    """odic_jpeg_any_decode on one 4:1:0 17x33 file with the workspace, the compressed-data copy, the RGB output and
    `status` each exactly as large as asked for inside a poisoned allocation: nothing outside them is written."""
    fresh, made = guarded_preprocessor(monkeypatch)
    name = "410-17x33"
    for knobs in ({}, dict(subseq_bits=32, max_sync_passes=0)):
        got, = fresh.decode_jpeg([L.CASES[name].blob], **ALL, **knobs)
        torch.cuda.synchronize()
        assert fresh.last_routes == ("device-layout",)
        assert np.array_equal(got.cpu().numpy(), L.oracle(L.CASES[name].blob))
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        for g in made:
            g.assert_untouched(what=f"layout decode, {g.dtype} buffer of {g.cols} elements")
        assert len([g for g in made if g.dtype == torch.uint8 and g.cols == 17 * 33 * 3]) == 1
        assert {g.dtype for g in made} == {torch.uint8, torch.int32}
        made.clear()


@pytest.mark.parametrize("draft", [None, (5, 6)], ids=["full", "draft"])
def test_jpeg_any_decode_stays_inside_its_buffers(both_counts, monkeypatch, draft):
    """odic_jpeg_any_decode / odic_jpeg_any_decode_scaled on one batch that holds both component counts (17x33 4:1:0,
    17x33 YCCK, 20x24 RGB 4:4:0; the draft request (5, 6) gives them scales 2, 2 and 4), every buffer exactly sized inside
    a poisoned allocation: the guards are untouched, and exactly the images' bytes and three status words are written —
    the bytes of the output between the images (each offset is rounded up to a multiple of 4) keep their poison."""
    blobs, hdrs = both_counts
    fresh, made = guarded_preprocessor(monkeypatch)
    called = []
    real_check = fresh._hip.check
    monkeypatch.setattr(fresh._hip, "check", lambda code, what: (called.append(what), real_check(code, what))[1])
    scales = [J.draft_scale((h.width, h.height), draft) if draft else 1 for h in hdrs]
    assert scales == ([2, 2, 4] if draft else [1, 1, 1])
    for knobs in ({}, dict(subseq_bits=32, max_sync_passes=0)):
        got = fresh.decode_jpeg(blobs, draft=draft, draft_layouts="all", **BOTH, **knobs)
        torch.cuda.synchronize()
        assert fresh.last_routes == ("device-layout", "device-cmyk", "device-layout")
        assert called == ["odic_jpeg_any_decode" + ("_scaled" if draft else "")]
        want = [drafted(b, s) for b, s in zip(blobs, scales)]
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g.cpu().numpy(), w), k
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        for g in made:
            g.assert_untouched(what=f"both counts, draft {draft}: {g.dtype} buffer of {g.cols} elements")
        offs, pos = [], 0
        for w in want:
            pos = (pos + 3) // 4 * 4
            offs.append(pos)
            pos += w.size
        rgb, = [g for g in made if g.dtype == torch.uint8 and g.cols == pos]
        flat = rgb.t.view(-1).cpu().numpy()
        gaps = np.ones(pos, bool)
        for o, w in zip(offs, want):
            gaps[o:o + w.size] = False
        assert gaps.any() and (flat[gaps] == POISON).all()
        status, = [g for g in made if g.dtype == torch.int32]
        assert status.cols == 3 and status.t.view(-1).cpu().tolist() == [0, 0, 0]
        made.clear()
        called.clear()


# ------------------------------------------------------------------------------------------------------------
# odic_jpeg_any_decode through the C ABI: both component counts in one call, containment, refused records
# ------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A
BOTH = dict(non_rgb="convert", cmyk="device", layouts="all")


@pytest.fixture(scope="module")
def both_counts():
    """17x33 4:1:0 (three components), 17x33 YCCK at Photoshop's 2x2 (four), 20x24 RGB-stored 4:4:0 (three)."""
    rgb440 = write_jpeg3(L.picture(24, 20, seed=3), [(1, 2), (1, 1), (1, 1)], "adobe0")
    blobs = [L.CASES["410-17x33"].blob, K.CASES["photoshop-ycck-2x2-17x33"][0], rgb440]
    hdrs = [J.parse(b, **BOTH) for b in blobs]
    assert [(h.kind, h.ncomp, h.width, h.height) for h in hdrs] == [("device", 3, 17, 33), ("device", 4, 17, 33),
                                                                  ("device", 3, 20, 24)]
    assert hdrs[1].ycck and hdrs[1].comp_hv[0] == (2, 2) and hdrs[2].rgb and hdrs[2].comp_hv[0] == (1, 2)
    return blobs, hdrs


def drafted(blob, scale):
    """Pillow's decode of the file at 1 / scale: `draft` with the request that picks exactly that scale."""
    im = Image.open(io.BytesIO(blob))
    if scale > 1:
        w, h = im.size
        im.draft("RGB", (w // scale, h // scale))
        assert im.size == J.scaled_size((w, h), scale)
    return np.asarray(im.convert("RGB"), dtype=np.uint8)


def run_any(pre, blobs, hdrs, scales=None, edit=None):
    """One odic_jpeg_any_decode call (scales: odic_jpeg_any_decode_scaled) on the files, the workspace, the RGB output and
    `status` each exactly as large as asked for inside a poisoned allocation (guards.py).  edit(rec): changes the packed
    records first.  → (status list, the output bytes, the output offsets, the guarded buffers)."""
    hip, lib, n, dev = pre._hip, pre.lib, len(blobs), "cuda:0"
    starts = np.cumsum([0] + [len(b) for b in blobs]).tolist()
    rec, tot, out_offs, out_bytes = J.pack_headers(hdrs, [o + h.data_offset for o, h in zip(starts, hdrs)], starts[1:],
                                                   2048, scales, dtype=J.HEADER_ANY_DTYPE)
    if edit is not None:
        edit(rec)
    batch = hip.JpegBatch()
    batch.n_images, batch.subseq_bits, batch.max_sync_passes = n, 2048, 4
    pre._set_fields(batch, tot)
    need = lib.odic_jpeg_any_workspace_bytes(ctypes.byref(batch))
    assert need > 0
    put = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(dev)
    drec, data = put(rec), put(np.frombuffer(b"".join(blobs), np.uint8))
    ws = guarded(1, need, need, torch.uint8, dev)
    out = guarded(1, out_bytes, out_bytes, torch.uint8, dev)
    out.t.fill_(SENTINEL)
    status = guarded(1, n, n, torch.int32, dev)
    batch.headers, batch.data, batch.out, batch.status = drec.data_ptr(), data.data_ptr(), out.data_ptr(), status.data_ptr()
    args, name = [ctypes.byref(batch), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream], "odic_jpeg_any_decode"
    if scales is not None:
        lg = torch.tensor([s.bit_length() - 1 for s in scales], dtype=torch.int32, device=dev)
        args.insert(1, lg.data_ptr())
        name += "_scaled"
    hip.check(getattr(lib, name)(*args), name)
    torch.cuda.synchronize()
    return status.t.view(-1).cpu().tolist(), out.t.view(-1).cpu().numpy(), out_offs, (ws, out, status)


@pytest.mark.parametrize("scales", [None, (1, 2, 8)], ids=["full", "scaled-1-2-8"])
def test_one_call_decodes_three_and_four_component_files(pre, both_counts, scales):
    """The path the merged record creates: no caller could put both counts into one call before.  Every image equals
    Pillow's `convert("RGB")` (after `draft` at its own scale), every status is 0, every buffer is exactly sized, and
    exactly the images' bytes are written: the padding between them keeps its sentinel."""
    blobs, hdrs = both_counts
    st, px, offs, bufs = run_any(pre, blobs, hdrs, list(scales) if scales else None)
    assert st == [0, 0, 0]
    written = np.zeros(len(px), bool)
    for k, (blob, off) in enumerate(zip(blobs, offs)):
        want = drafted(blob, scales[k] if scales else 1)
        assert off % 4 == 0 and np.array_equal(px[off:off + want.size].reshape(want.shape), want), k
        written[off:off + want.size] = True
    assert (px[~written] == SENTINEL).all() and (~written).sum() == len(px) - sum(drafted(b, s).size for b, s in
                                                                                 zip(blobs, scales or (1, 1, 1)))
    for g in bufs:
        g.assert_untouched(what=f"mixed counts, scales {scales}: {g.dtype} buffer of {g.cols} elements")


def _set(field, c, value):
    def edit(rec):
        rec[field][0, c] = value
    edit.__name__ = f"{field}{c}={value}"
    return edit


def _ncomp(value):
    def edit(rec):
        rec["ncomp"][0] = value
    edit.__name__ = f"ncomp={value}"
    return edit


def _not_a_divisor(rec):                                     # 3x2 + 2x1 + 1x1: nine blocks, and 2 does not divide 3
    rec["h"][0, 0], rec["h"][0, 1] = 3, 2


def _eleven_blocks(rec):                                     # 4x2 + 2x1 + 1x1: every factor divides the largest
    rec["h"][0, 1] = 2


# (file, edit of its packed record): a factor of 5, a factor that does not divide the largest, 11 blocks per MCU; then the
# four-component rules: a component count that is none, component 0 at 3x1, a component at neither 1x1 nor component 0's
REFUSED = [("410-17x33", _set("h", 0, 5)), ("410-17x33", _not_a_divisor), ("410-17x33", _eleven_blocks),
           ("photoshop-ycck-2x2-17x33", _ncomp(2)), ("photoshop-ycck-2x2-17x33", _ncomp(5)),
           ("photoshop-ycck-2x2-17x33", _set("h", 0, 3)), ("photoshop-ycck-2x2-17x33", _set("v", 3, 1))]


@pytest.mark.parametrize("name,edit", REFUSED, ids=[e.__name__ for _, e in REFUSED])
@pytest.mark.parametrize("scaled", [False, True], ids=["full", "scaled"])
def test_refused_records_write_nothing(pre, name, edit, scaled):
    """A record that breaks the frame rules, made by editing the packed record of a valid 17x33 file, with the buffers
    sized for the valid file: status 1, the output keeps its sentinel, nothing outside the buffers is touched."""
    blob = L.CASES[name].blob if name in L.CASES else K.CASES[name][0]
    hd = J.parse(blob, **BOTH)
    st, px, _, bufs = run_any(pre, [blob], [hd], [1] if scaled else None, edit)
    assert st == [1] and (px == SENTINEL).all()
    for g in bufs:
        g.assert_untouched(what=edit.__name__)
    if edit is REFUSED[0][1] and not scaled:                 # the unedited records decode
        for n in ("410-17x33", "photoshop-ycck-2x2-17x33"):
            b = L.CASES[n].blob if n in L.CASES else K.CASES[n][0]
            st, px, _, _ = run_any(pre, [b], [J.parse(b, **BOTH)])
            assert st == [0] and np.array_equal(px.reshape(33, 17, 3), L.oracle(b))
