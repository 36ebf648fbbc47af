"""`non_rgb="convert"` on the GPU: one-component JPEGs through odic_jpeg_decode / odic_jpeg_decode_progressive and
their _scaled forms (DevicePreprocessor.decode_jpeg / from_jpeg_bytes / from_files) against Pillow's
`Image.open(f).convert("RGB")`, bit for bit; the other non-RGB kinds on the host route; and the default, unchanged."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import guards
import jpeg_gray_cases as G
from on_device_image_captioning_amd import jpeg as J
from test_jpeg_host import encode, smooth_rgb

pytestmark = pytest.mark.gpu

KNOBS = {"default": dict(), "subseq32": dict(subseq_bits=32), "serial": dict(max_sync_passes=0),
         "subseq32-serial": dict(subseq_bits=32, max_sync_passes=0)}
ROUTE = {k: "device-progressive" if k.startswith("progressive") else "device" for k in G.KINDS}
CONVERT = dict(progressive="device", non_rgb="convert")


@pytest.fixture(scope="module")
def pre():
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)


@pytest.fixture(scope="module")
def small():
    """Input size 16: the sizes used here are large enough for draft=True to pick a scale."""
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    return DevicePreprocessor(16, "cuda:0", max_pixels=512 * 512)


def decode_and_compare(pre, blobs, draft=None, **kw):
    got = pre.decode_jpeg(blobs, draft=draft, **kw)
    assert len(got) == len(blobs)
    for k, (g, b) in enumerate(zip(got, blobs)):
        want = G.pil_convert(b, draft)
        g = g.cpu().numpy()
        assert g.shape == want.shape, (k, g.shape, want.shape)
        assert np.array_equal(g, want), (k, pre.last_routes[k], int(np.abs(g.astype(int) - want).max()))
    return pre.last_routes


# ---------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", KNOBS)
def test_exactness_matrix(pre, knobs):
    cases = [(kind, size) for kind in G.KINDS for size in G.SIZES]
    blobs = [G.gray_file(kind, size) for kind, size in cases]
    routes = decode_and_compare(pre, blobs, **CONVERT, **KNOBS[knobs])
    assert list(routes) == [ROUTE[kind] for kind, _ in cases]                    # exact, and not by the host's doing
    for blob, (kind, size) in zip(blobs[::7], cases[::7]):                       # ... and alone
        assert decode_and_compare(pre, [blob], **CONVERT, **KNOBS[knobs]) == (ROUTE[kind],)


def test_progressive_gray_takes_the_host_route_unless_asked(pre):
    blobs = [G.gray_file("progressive", (37, 53)), G.gray_file("baseline", (37, 53))]
    assert decode_and_compare(pre, blobs, non_rgb="convert") == ("host", "device")


@pytest.mark.parametrize("kind", ["baseline", "dri3", "progressive"])
def test_patched_files(pre, kind):
    """libjpeg ignores the sampling factors and the component id a one-component SOF declares."""
    blobs, originals = [], []
    for size in [(9, 17), (37, 53)]:
        blob = G.gray_file(kind, size)
        patched = [G.patch_hv(blob, hv) for hv in G.HV_PATCHES] + [G.patch_id(blob)]
        blobs += patched
        originals += [blob] * len(patched)
    routes = decode_and_compare(pre, blobs, **CONVERT)
    assert set(routes) == {ROUTE[kind]}
    for a, b in zip(blobs, originals):
        assert a != b and np.array_equal(G.pil_convert(a), G.pil_convert(b))


@pytest.mark.parametrize("s", [2, 4, 8])
def test_draft(pre, s):
    kinds = ["baseline", "noise100", "dri3", "progressive", "progressive-dri3"]
    for size in [(64, 48), (65, 47), (9, 17)]:
        req = (max(size[0] // s, 1), max(size[1] // s, 1))
        assert J.draft_scale(size, req) == s
        blobs = [G.gray_file(kind, size) for kind in kinds]
        routes = decode_and_compare(pre, blobs, draft=req, **CONVERT)
        assert list(routes) == [ROUTE[k] for k in kinds]
        want = (-(-size[1] // s), -(-size[0] // s), 3)
        assert all(G.pil_convert(b, req).shape == want for b in blobs)


def test_mixed_scales_in_one_call(pre):
    sizes = [(20, 24), (40, 33), (70, 77), (130, 129), (31, 200)]
    blobs = []
    for k, size in enumerate(sizes):
        blobs.append(G.gray_file("dri3" if k % 2 else "baseline", size))
        blobs.append(G.gray_file("progressive", size, seed=1))
        blobs.append(encode(smooth_rgb(size[1], size[0], seed=k), quality=90, subsampling=k % 3))
    routes = decode_and_compare(pre, blobs, draft=(16, 16), **CONVERT)
    assert routes == ("device", "device-progressive", "device") * len(sizes)
    assert [J.draft_scale(s, (16, 16)) for s in sizes] == [1, 2, 4, 8, 1]


# ---------------------------------------------------------------------------------------------------------------
# mixed batches
# ---------------------------------------------------------------------------------------------------------------
def mixed_blobs():
    out = [("444", encode(smooth_rgb(48, 64, seed=1), quality=90, subsampling=0)),
           ("gray", G.gray_file("dri3", (65, 47))),
           ("422", encode(smooth_rgb(47, 65, seed=2), quality=90, subsampling=1)),
           ("gray-progressive", G.gray_file("progressive", (64, 48))),
           ("cmyk", G.cmyk_jpeg(48, 64)),
           ("420", encode(smooth_rgb(33, 70, seed=3), quality=90, subsampling=2)),
           ("gray", G.gray_file("noise100", (37, 53)))]
    return [n for n, _ in out], [b for _, b in out]


MIXED_ROUTES = {"444": "device", "422": "device", "420": "device", "gray": "device",
                "gray-progressive": "device-progressive", "cmyk": "host", "png": "host"}


@pytest.mark.parametrize("draft", [None, (16, 16)], ids=["full", "drafted"])
def test_mixed_batch_keeps_input_order(pre, draft):
    names, blobs = mixed_blobs()
    routes = decode_and_compare(pre, blobs, draft=draft, **CONVERT)
    assert list(routes) == [MIXED_ROUTES[n] for n in names]
    routes = decode_and_compare(pre, blobs, draft=draft, non_rgb="convert")      # progressive="host"
    assert list(routes) == ["host" if n == "gray-progressive" else MIXED_ROUTES[n] for n in names]


def test_from_files_device_equals_host(small, tmp_path):
    names, blobs = mixed_blobs()
    names += ["png", "png"]
    blobs += [G.png("L", 48, 64), G.png("RGBA", 40, 50)]
    paths = []
    for k, b in enumerate(blobs):
        p = tmp_path / f"f{k}.{'png' if names[k] == 'png' else 'jpg'}"
        p.write_bytes(b)
        paths.append(str(p))
    regions = [(1, (3.5, 2.0, 40.25, 30.0)), (7, (0, 0, 64, 48)), (4, (10, 5, 33.5, 20)), (3, (1, 1, 9, 9)),
               (8, (2.5, 2.5, 30, 30))]
    for kw in (dict(), dict(draft=True)):
        host = small.from_files(paths, decode="host", non_rgb="convert", **kw)
        dev = small.from_files(paths, decode="device", non_rgb="convert", **kw)
        # from_files has no `progressive`: the gray progressive file goes to PIL
        assert list(small.last_routes) == ["host" if n == "gray-progressive" else MIXED_ROUTES[n] for n in names]
        assert torch.equal(dev, host)
        arrays = [G.pil_convert(b, (16, 16) if kw else None).copy() for b in blobs]
        assert torch.equal(host, small(arrays))                                  # ... and both are Pillow's pixels
        via_bytes = small.from_jpeg_bytes(blobs, non_rgb="convert", progressive="device", **kw)
        assert small.last_routes[3] == "device-progressive" and torch.equal(via_bytes, host)
    # regions: boxes inside the smallest drafted image are inside all of them
    boxes = [(i, (0.5, 1.0, 4.5, 5.0)) for i in (1, 3, 4, 7, 8, 0)]
    for kw, reg in ((dict(), regions), (dict(draft=True), boxes)):
        host = small.from_files(paths, decode="host", non_rgb="convert", regions=reg, **kw)
        dev = small.from_files(paths, decode="device", non_rgb="convert", regions=reg, **kw)
        assert host.shape == (len(reg), 3, 16, 16) and torch.equal(dev, host)
        assert torch.equal(small.from_jpeg_bytes(blobs, non_rgb="convert", regions=reg, **kw), host)


@pytest.mark.parametrize("draft", [None, (16, 16)], ids=["full", "drafted"])
def test_default_is_unchanged(pre, small, draft, tmp_path):
    """non_rgb="black", or no keyword: black canvases of the right (drafted) size, route "black"."""
    names, blobs = mixed_blobs()
    runs = [pre.decode_jpeg(blobs, draft=draft, progressive="device"),
            pre.decode_jpeg(blobs, draft=draft, progressive="device", non_rgb="black")]
    for got in runs:
        assert list(pre.last_routes) == ["device" if n[0] == "4" else "black" for n in names]
    for k, (name, blob) in enumerate(zip(names, blobs)):
        im = Image.open(io.BytesIO(blob))
        if draft is not None:
            im.draft("RGB", draft)
        want = np.asarray(im) if im.mode == "RGB" else np.zeros(im.size[::-1] + (3,), np.uint8)
        for got in runs:
            assert got[k].dtype == torch.uint8 and np.array_equal(got[k].cpu().numpy(), want), (k, name)
    paths = []
    for k, b in enumerate(blobs + [G.png("L", 48, 64)]):
        p = tmp_path / f"f{k}"
        p.write_bytes(b)
        paths.append(str(p))
    kw = dict(draft=True) if draft else dict()
    host = small.from_files(paths, **kw)
    assert torch.equal(small.from_files(paths, decode="device", **kw), host)
    assert small.last_routes[-1] == "host" and set(small.last_routes[:-1]) == {"device", "black"}
    assert torch.equal(small.from_files(paths, decode="device", non_rgb="black", **kw), host)
    assert torch.equal(small.from_files(paths, decode="host", non_rgb="black", **kw), host)
    black = small([np.zeros((8, 8, 3), np.uint8)])[0]
    assert torch.equal(host[1], black) and torch.equal(host[-1], black)          # the gray JPEG and the L PNG
    assert not torch.equal(small.from_files(paths, non_rgb="convert", **kw)[1], black)


def test_size_check_and_its_order(tmp_path):
    """A gray file too large for the staging buffers goes to PIL like any oversized file, and the size check of
    `__call__` then fails on both routes; PIL's own exception for an earlier file comes first."""
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    tiny = DevicePreprocessor(16, "cuda:0", max_pixels=32 * 32)
    big, ok = G.gray_file("baseline", (37, 53)), G.gray_file("baseline", (9, 17))
    assert [tuple(t.shape) for t in tiny.decode_jpeg([ok], non_rgb="convert")] == [(17, 9, 3)]
    for blobs, err in (([ok, big], RuntimeError), ([G.truncated(ok), big], OSError), ([big, G.truncated(ok)], OSError)):
        errs = []
        for decode in ("host", "device"):
            paths = []
            for k, b in enumerate(blobs):
                (tmp_path / f"{k}.jpg").write_bytes(b)
                paths.append(str(tmp_path / f"{k}.jpg"))
            with pytest.raises(Exception) as e:
                tiny.from_files(paths, decode=decode, non_rgb="convert")
            errs.append(e.value)
        assert type(errs[0]) is type(errs[1]) and isinstance(errs[0], err) and str(errs[0]) == str(errs[1])


# ---------------------------------------------------------------------------------------------------------------
# containment
# ---------------------------------------------------------------------------------------------------------------
def test_gray_decode_stays_inside_its_buffers(monkeypatch):
    """As test_jpeg_decode_stays_inside_its_workspace and test_scaled_decode_stays_inside_its_buffers, for gray batches
    and batches that mix gray and colour: the workspace, the data copy, the RGB output and `status` are exactly the
    requested bytes inside poisoned allocations; the output holds the images' H·W·3 (drafted) bytes and nothing else."""
    from on_device_image_captioning_amd import image_utils
    from on_device_image_captioning_amd.image_utils import DevicePreprocessor
    made = []
    orig = DevicePreprocessor._grow

    def exact(buf, nbytes, **kw):
        if "device" not in kw:
            return orig(buf, nbytes, **kw)
        g = guards.guarded(1, max(nbytes, 1), max(nbytes, 1), torch.uint8, kw["device"])
        made.append(g)
        return g.t.view(-1)

    class TorchWithGuardedEmpty:
        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty(*size, **kw):
            if kw.get("device") is not None and not kw.get("pin_memory") and len(size) == 1 and isinstance(size[0], int) \
                    and kw.get("dtype") in (torch.uint8, torch.int32) and torch.device(kw["device"]).type == "cuda":
                g = guards.guarded(1, size[0], size[0], kw["dtype"], kw["device"])
                made.append(g)
                return g.t.view(-1)
            return torch.empty(*size, **kw)

    monkeypatch.setattr(DevicePreprocessor, "_grow", staticmethod(exact))
    pre = DevicePreprocessor(384, "cuda:0", max_pixels=512 * 512)
    monkeypatch.setattr(image_utils, "torch", TorchWithGuardedEmpty())
    base = [G.gray_file(k, s) for k, s in (("baseline", (1, 1)), ("dri3", (37, 53)), ("noise100", (9, 17)),
                                           ("optimize", (65, 47)))]
    prog = [G.gray_file(k, s) for k, s in (("progressive", (37, 53)), ("progressive-dri3", (7, 9)),
                                           ("progressive", (64, 48)))]
    colour = [encode(smooth_rgb(33, 70, seed=3), quality=90, subsampling=2)]
    kinds = set()
    for batch, req in ((base, None), (prog, None), (base + prog + colour, None), (base[:1], None),
                       (base + prog + colour, (16, 16)), (base, (4, 4)), (prog, (9, 12)), (prog + base, (1, 1))):
        routes = decode_and_compare(pre, batch, draft=req, **CONVERT)
        assert set(routes) <= {"device", "device-progressive"}
        torch.cuda.synchronize()
        dev, pinned = pre._jpeg_dev, pre._jpeg_pinned
        n = min(dev.numel(), pinned.numel())
        assert n >= sum(len(b) for b in batch) and torch.equal(dev[:n].cpu(), pinned[:n]), "inputs are only read"
        assert len(made) >= 4, "workspace, data copy, RGB output and status are all guarded"
        out_bytes = sum(int(np.prod(G.pil_convert(b, req).shape)) for b in batch)
        assert any(g.dtype == torch.uint8 and g.cols == out_bytes for g in made), "the output holds the images only"
        assert any(g.dtype == torch.int32 and g.cols == len(batch) for g in made)
        for g in made:
            g.assert_untouched(what=f"gray jpeg decode, draft {req}, {g.dtype} buffer of {g.cols} elements")
            kinds.add(g.dtype)
        made.clear()
    assert kinds == {torch.uint8, torch.int32}


# ---------------------------------------------------------------------------------------------------------------
# damaged streams: status 1, then whatever the host route does with the file.  The decoder's walks over a gray stream
# are the ones it makes over a colour stream, with the same bounds: the segment pass reads the file's own bytes, a
# unit's decode ends at the unit's last bit, the write-out stops at the interval's last block, the serial walk visits
# the interval's units once, and a progressive scan checks pos <= end before every symbol.
# ---------------------------------------------------------------------------------------------------------------
DAMAGED = {
    "truncated scan": lambda: G.truncated(G.gray_file("baseline", (37, 53))),
    "truncated scan, restart markers": lambda: G.truncated(G.gray_file("dri3", (37, 53))),
    "invalid code": lambda: G.invalid_code(G.gray_file("noise100", (37, 53))),
    "invalid code, restart markers": lambda: G.invalid_code(G.gray_file("dri3", (65, 47))),
    "RST out of sequence": lambda: G.rst_out_of_sequence(G.gray_file("dri3", (37, 53))),
    "RST out of sequence, one block per interval": lambda: G.rst_out_of_sequence(G.gray_file("dri1", (9, 17))),
}


@pytest.mark.parametrize("knobs", ["default", "subseq32-serial"])
@pytest.mark.parametrize("name", DAMAGED)
def test_damaged_gray_streams_fall_back_to_the_host(pre, name, knobs):
    bad = DAMAGED[name]()
    assert J.parse(bad, "convert").kind == J.DEVICE                              # the header is whole
    good = G.gray_file("baseline", (9, 17))
    try:
        want = G.pil_convert(bad)
    except Exception as e:                                                       # the host route's exception, in its order
        with pytest.raises(type(e)) as got:
            pre.decode_jpeg([good, bad], non_rgb="convert", **KNOBS[knobs])
        assert str(got.value) == str(e)
        assert pre.last_routes == ("device", "host-after-status")
        return
    got = pre.decode_jpeg([good, bad], non_rgb="convert", **KNOBS[knobs])
    assert pre.last_routes == ("device", "host-after-status")
    assert np.array_equal(got[1].cpu().numpy(), want) and np.array_equal(got[0].cpu().numpy(), G.pil_convert(good))
    if "truncated" not in name:
        for draft in ((9, 8), (4, 5)):
            got = pre.decode_jpeg([bad], draft=draft, non_rgb="convert", **KNOBS[knobs])
            assert pre.last_routes == ("host-after-status",)
            assert np.array_equal(got[0].cpu().numpy(), G.pil_convert(bad, draft))


def test_damaged_progressive_gray_stream(pre):
    blob = G.gray_file("progressive-dri3", (37, 53))
    hd = J.parse_progressive(blob, "convert")
    sc = hd.scans[-1]
    at = blob.index(b"\xff\xd0", sc.data_offset, sc.data_end)
    bad = blob[:at] + b"\xff\xd3" + blob[at + 2:]                                # RST0 → RST3 in the last scan
    assert J.parse_progressive(bad, "convert").kind == J.DEVICE
    want = G.pil_convert(bad)
    got = pre.decode_jpeg([bad, blob], **CONVERT)
    assert pre.last_routes == ("host-after-status", "device-progressive")
    assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), G.pil_convert(blob))
