"""Caller-side image preprocessing (reference utils/image_utils.py:5-23).

torchvision is not installed in this image, so the three transforms are spelled out with PIL and
torch: Resize((S,S)) on a PIL image is `Image.resize((S,S), BILINEAR)`, ToTensor is HWC uint8 → CHW
float /255, Normalize is the ImageNet mean/std.  Non-RGB files become an all-black RGB canvas, as
the reference does (it calls PIL_Image.new, image_utils.py:18-19).
"""
from __future__ import annotations

import ctypes
import io

import numpy as np
import torch
from PIL import Image

from .jpeg import pad256 as _pad256

_MEAN = (0.485, 0.456, 0.406)
_STD = (0.229, 0.224, 0.225)


def preprocess_image(image_path: str, img_size: int) -> torch.Tensor:
    pil = Image.open(image_path)
    if pil.mode != "RGB":
        pil = Image.new("RGB", pil.size)
    pil = pil.resize((img_size, img_size), Image.BILINEAR)
    chw = torch.from_numpy(np.asarray(pil, dtype=np.uint8).copy()).permute(2, 0, 1).to(torch.float32) / 255.0
    mean = torch.tensor(_MEAN, dtype=torch.float32).view(3, 1, 1)
    std = torch.tensor(_STD, dtype=torch.float32).view(3, 1, 1)
    return ((chw - mean) / std).unsqueeze(0)


# =================================================================================================
# Device-side pipeline: resize + ToTensor + Normalize on the GPU, bit-exact with the
# PIL / torch path above; pinned double-buffered uploads so the copy of image i+1 overlaps the
# kernels of image i.  Baseline and progressive JPEGs can also be decoded on the GPU (odic_jpeg_decode /
# odic_jpeg_decode_progressive, csrc/jpeg_decode.hip), bit-exact with PIL: `from_jpeg_bytes` /
# `from_files(..., decode="device")`.  Files the device decoder does not take (arithmetic coding, non-JPEG, ...)
# and images whose entropy data fails to decode are decoded by PIL in the same call, so the result and the
# exceptions are those of the host path.  With a draft request (`draft=`) the files are decoded at 1/2, 1/4 or 1/8 scale
# in the DCT domain, as `PIL.Image.draft` does, on either path and bit-exact between them.  Non-RGB files are a black
# canvas as in the reference, or with `non_rgb="convert"` what `convert("RGB")` makes of them: grayscale JPEGs on the
# device, the other modes by PIL.  With `orientation="exif"` every image is turned upright as `ImageOps.exif_transpose`
# does: device-decoded files by one odic_orient_rgb8 launch (csrc/orient.hip), PIL-decoded ones by PIL.  With
# `cmyk="device"` (and `non_rgb="convert"`) baseline CMYK / YCCK JPEGs are decoded and converted on the device too
# (odic_jpeg_any_decode) instead of leaving the batch for PIL.  With `layouts="all"` so are baseline three-component
# JPEGs at the sampling layouts and colour spaces the common decode turns away (the same call: 4:4:0, 4:1:1,
# 4:1:0, RGB-stored files, ...).  With `progressive="device"` beside either keyword the progressive files of that kind are
# decoded on the device as well (odic_jpeg_decode_progressive_any).  Under a draft request those four kinds go to PIL
# unless `draft_layouts="all"`, which decodes them at the draft scale on the device (the two _scaled entry points).
# =================================================================================================
_PRECISION_BITS = 32 - 8 - 2


def pil_bilinear_coeffs(in_size: int, out_size: int):
    """Tap windows and fixed-point weights of PIL's BILINEAR resampler for one axis, computed exactly as
    libImaging/Resample.c::precompute_coeffs + normalize_coeffs_8bpc do (double arithmetic, taps summed in
    order): → (bounds int32 [out, 2] = first tap / tap count, coeffs int32 [out, ksize], ksize)."""
    return pil_bilinear_coeffs_box(in_size, 0, in_size, out_size)


def pil_bilinear_coeffs_box(in_size: int, in0: float, in1: float, out_size: int):
    """The same for the span [in0, in1) of an axis of in_size pixels: one axis of `Image.resize(size, BILINEAR, box=)`.
    Pillow carries the box as C floats: both ends are rounded to float32 and their difference is taken in float32,
    everything after that is double.  The tap windows are clipped to the image, not to the box, so pixels just outside
    the box contribute at its edges.  ValueError unless 0 <= in0 < in1 <= in_size (after the rounding)."""
    in_size, out_size = int(in_size), int(out_size)
    f0, f1 = np.float32(in0), np.float32(in1)
    if not (0 <= f0 < f1 <= in_size) or out_size <= 0:
        raise ValueError(f"box span [{in0}, {in1}) must satisfy 0 <= start < end <= {in_size}")
    scale = float(f1 - f0) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale                              # bilinear filter support = 1
    ksize = int(np.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = float(f0) + (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C (int) cast: truncation, values >= -0.5
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    n = xmax - xmin
    ss = 1.0 / filterscale
    taps = np.arange(ksize, dtype=np.float64)[None, :]
    arg = np.abs((taps + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where(arg < 1.0, 1.0 - arg, 0.0)
    w = np.where(taps < n[:, None], w, 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for i in range(ksize):                                                    # same summation order as the C loop
        ww = ww + w[:, i]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fixed = np.where(w < 0, -0.5 + w * (1 << _PRECISION_BITS), 0.5 + w * (1 << _PRECISION_BITS)).astype(np.int64)
    fixed = np.where(taps < n[:, None], fixed, 0).astype(np.int32)
    bounds = np.stack([xmin, n], axis=1).astype(np.int32)
    return bounds, fixed, ksize


#: odic_resize_job (include/odic_hip.h), field for field
RESIZE_JOB_DTYPE = np.dtype([("src_off", "<i8"), ("src_pitch", "<i8"), ("tmp_off", "<i8"), ("H", "<i4"), ("W", "<i4"),
                             ("row_first", "<i4"), ("n_rows", "<i4"), ("bounds_x", "<i4"), ("coef_x", "<i4"),
                             ("bounds_y", "<i4"), ("coef_y", "<i4"), ("ksize_x", "<i4"), ("ksize_y", "<i4")])
MAX_RESIZE_JOBS = 65535                                       # one grid z index per job
#: odic_orient_job (include/odic_hip.h), field for field; the C struct's trailing padding included
ORIENT_JOB_DTYPE = np.dtype([("src_off", "<i8"), ("dst_off", "<i8"), ("src_stride_bytes", "<i8"), ("H", "<i4"),
                             ("W", "<i4"), ("orientation", "<i4")], align=True)


def pack_resize_jobs(jobs, out_size: int):
    """jobs: sequence of (src_off, H, W, src_pitch, (l, t, r, b)) — the byte offset of an RGB8 image in one buffer, its
    size and row pitch in bytes, and a box as `Image.resize` takes it → (records RESIZE_JOB_DTYPE [N], bounds pool
    int32, coefficient pool int32, tmp_bytes, max_rows) for odic_resize_boxes_normalize.  Axes with the same
    (in_size, in0, in1) after the float32 rounding share one table in the pools.  This is where the geometry is
    validated (the kernel trusts the records): ValueError for a box outside 0 <= l < r <= W, 0 <= t < b <= H, a pitch
    below 3 W or a negative offset."""
    S = int(out_size)
    if not 1 <= S <= 65535:
        raise ValueError(f"out_size must lie in 1..65535, not {out_size}")
    if len(jobs) > MAX_RESIZE_JOBS:
        raise ValueError(f"at most {MAX_RESIZE_JOBS} regions per call, not {len(jobs)}")
    rec = np.zeros(len(jobs), RESIZE_JOB_DTYPE)
    axes, bounds, coefs = {}, [], []
    n_bounds = n_coefs = 0

    def axis(in_size, in0, in1):
        nonlocal n_bounds, n_coefs
        key = (in_size, float(np.float32(in0)), float(np.float32(in1)))
        if key not in axes:
            b, k, ks = pil_bilinear_coeffs_box(in_size, in0, in1, S)
            axes[key] = (n_bounds, n_coefs, ks, int(b[0, 0]), int(b[-1, 0] + b[-1, 1]))
            bounds.append(b.reshape(-1))
            coefs.append(k.reshape(-1))
            n_bounds += b.size
            n_coefs += k.size
        return axes[key]

    tmp_bytes = max_rows = 0
    for r, (src_off, H, W, pitch, box) in zip(rec, jobs):
        src_off, H, W, pitch = int(src_off), int(H), int(W), int(pitch)
        if len(box) != 4:
            raise ValueError(f"a box is (left, top, right, bottom), not {box!r}")
        if H <= 0 or W <= 0 or H > 65535 or pitch < 3 * W or src_off < 0:
            raise ValueError(f"bad source image: {H} x {W}, pitch {pitch}, offset {src_off}")
        try:
            bx, kx, ksx, _, _ = axis(W, box[0], box[2])
            by, ky, ksy, first, last = axis(H, box[1], box[3])
        except ValueError:
            raise ValueError(f"box {tuple(box)!r} does not fit a {W} x {H} image: 0 <= left < right <= width and "
                             "0 <= top < bottom <= height are required") from None
        r["src_off"], r["src_pitch"], r["tmp_off"], r["H"], r["W"] = src_off, pitch, tmp_bytes, H, W
        r["row_first"], r["n_rows"] = first, last - first
        r["bounds_x"], r["coef_x"], r["ksize_x"] = bx, kx, ksx
        r["bounds_y"], r["coef_y"], r["ksize_y"] = by, ky, ksy
        tmp_bytes += (last - first) * S * 3
        max_rows = max(max_rows, last - first)
    if n_bounds >= 2 ** 31 or n_coefs >= 2 ** 31:
        raise ValueError("too many distinct boxes for one call: the coefficient pool is indexed with int32")
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return rec, cat(bounds), cat(coefs), tmp_bytes, max_rows


class DevicePreprocessor:
    """Batched `preprocess_image` on the GPU: host-decoded RGB arrays → fp32 [B, 3, S, S].

        pre = DevicePreprocessor(384, device)
        batch = pre([np.asarray(PIL.Image.open(f).convert_or_black()) ...])     # or pre.from_files(paths)
    """

    def __init__(self, img_size: int, device, max_pixels: int = 4608 * 3456):
        from . import _hip
        self._hip = _hip
        self.lib = _hip.load()
        self.S, self.device = img_size, torch.device(device)
        self.max_bytes = max_pixels * 3
        self.host = [torch.empty(self.max_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty(self.max_bytes, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.tmp = [torch.empty(0, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.ev = [torch.cuda.Event() for _ in range(2)]
        self.stream = torch.cuda.Stream(device=self.device)
        self._coef_cache = {}
        # device JPEG decode: grow-only pinned staging / device copies of the compressed batch, workspace
        self._jpeg_ev = torch.cuda.Event()
        self._jpeg_pinned = self._jpeg_dev = self._jpeg_ws = self._jpeg_status = None
        self._jpeg_tmp = torch.empty(0, dtype=torch.uint8, device=self.device)
        self._jpeg_routes, self._jpeg_prog_coef = [], None
        self._jpeg_orientations = []
        # region resize: grow-only gather buffer for images that do not share one storage, and the horizontal pass's rows
        self._region_src = self._region_tmp = None
        self._mean = (ctypes.c_float * 3)(*_MEAN)
        self._std = (ctypes.c_float * 3)(*_STD)

    def _coeffs(self, n: int):
        c = self._coef_cache.get(n)
        if c is None:
            b, k, ks = pil_bilinear_coeffs(n, self.S)
            c = (torch.from_numpy(b).to(self.device), torch.from_numpy(k).to(self.device), ks)
            self._coef_cache[n] = c
        return c

    def _check_size(self, H: int, W: int) -> None:
        if H * W * 3 > self.max_bytes:
            raise RuntimeError(f"image {H}x{W} exceeds the staging buffers ({self.max_bytes} bytes)")

    def _resize_whole(self, src_ptr: int, H: int, W: int, tmp: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
        """Resize + normalise the packed RGB8 image of H x W at device address src_ptr into dst fp32 [3,S,S], on
        self.stream.  tmp holds the horizontal pass's H x S pixels: → tmp, or a larger buffer that replaces it."""
        if tmp.numel() < H * self.S * 3:
            tmp = torch.empty(H * self.S * 3, dtype=torch.uint8, device=self.device)
        bx, kx, ksx = self._coeffs(W)
        by, ky, ksy = self._coeffs(H)
        self._hip.check(self.lib.odic_resize_bilinear_normalize(
            src_ptr, H, W, 3 * W, bx.data_ptr(), kx.data_ptr(), ksx, by.data_ptr(), ky.data_ptr(), ksy, tmp.data_ptr(),
            dst.data_ptr(), self.S, self._mean, self._std, self.stream.cuda_stream), "odic_resize_bilinear_normalize")
        return tmp

    def __call__(self, images) -> torch.Tensor:
        """images: sequence of HWC uint8 RGB numpy arrays (any sizes) → normalised fp32 [B,3,S,S] on the device,
        ordered after the work on the CURRENT stream."""
        S = self.S
        out = torch.empty(len(images), 3, S, S, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for i, img in enumerate(images):
                img = np.ascontiguousarray(img, dtype=np.uint8)
                if img.ndim != 3 or img.shape[2] != 3:
                    raise RuntimeError("DevicePreprocessor wants HWC RGB uint8 arrays")
                H, W, _ = img.shape
                self._check_size(H, W)
                nbytes = H * W * 3
                slot = i & 1
                self.ev[slot].synchronize()                                   # the kernels that read this slot are done
                self.host[slot][:nbytes].copy_(torch.from_numpy(img).reshape(-1))
                self.dev[slot][:nbytes].copy_(self.host[slot][:nbytes], non_blocking=True)
                self.tmp[slot] = self._resize_whole(self.dev[slot].data_ptr(), H, W, self.tmp[slot], out[i])
                self.ev[slot].record(self.stream)
        torch.cuda.current_stream().wait_stream(self.stream)
        return out

    def from_files(self, paths, decode: str = "host", draft: bool = False, regions=None,
                   non_rgb: str = "black", orientation: str = "ignore", cmyk: str = "host",
                   layouts: str = "common", draft_layouts: str = "common") -> torch.Tensor:
        """JPEG/PNG files → fp32 [B,3,S,S].  decode="host": PIL decode (non-RGB files become a black canvas as in
        the reference) + device pipeline; decode="device": the file bytes go to `from_jpeg_bytes` (same result).
        non_rgb="convert": a file of any other mode (L, LA, P, RGBA, I;16, CMYK, ...) is read as
        `Image.open(f).convert("RGB")` instead of the black canvas, after the draft if there is one; with
        decode="device" baseline grayscale JPEGs are decoded on the device, everything else non-RGB by PIL.
        draft=True: JPEGs are decoded at the scale `Image.draft("RGB", (S, S))` picks (1/2, 1/4 or 1/8 while both sides
        stay at least S) and resized from there; the tensor differs slightly from the undrafted one, identically for
        both values of `decode`.
        regions: a sequence of (file index, (l, t, r, b)) → the region batch fp32 [N,3,S,S] of `resize_regions` instead
        of the whole-image batch, for either value of `decode` (torch.equal between them); with draft=True the boxes
        are in the coordinates of the drafted image.
        orientation="exif": every file, of any format, is turned upright by its EXIF Orientation tag as
        `ImageOps.exif_transpose` does, after the draft and the non-RGB rule (the black canvas has the transposed size),
        for either value of `decode` (torch.equal between them); region boxes are in oriented coordinates.  The default
        "ignore" reads the stored pixel grid, as the reference does.
        cmyk="device" (needs non_rgb="convert"): with decode="device" it is passed on to `from_jpeg_bytes`, where
        baseline CMYK / YCCK JPEGs are decoded on the device (under a draft request only with draft_layouts="all");
        decode="host" ignores it.  The tensor is the same either way.
        layouts="all": likewise passed on to `from_jpeg_bytes` with decode="device", where baseline three-component
        JPEGs at any sampling layout libjpeg decodes, and RGB-stored ones, are decoded on the device (under a draft
        request only with draft_layouts="all"); decode="host" ignores it.  The tensor is the same either way.
        draft_layouts="all": with decode="device" and draft=True the files of cmyk= and layouts= are decoded on the
        device at the draft scale instead of going to PIL (`decode_jpeg`); decode="host" ignores it, and so does a call
        without a draft.  The tensor is the same either way."""
        from .jpeg import check_cmyk, check_draft_layouts, check_layouts, check_non_rgb, check_orientation
        check_non_rgb(non_rgb)
        check_orientation(orientation)
        check_cmyk(cmyk, non_rgb)
        check_layouts(layouts)
        check_draft_layouts(draft_layouts)
        exif = {} if orientation == "ignore" else {"orientation": orientation}   # the default's calls stay as they are
        if cmyk != "host":
            exif["cmyk"] = cmyk
        if layouts != "common":
            exif["layouts"] = layouts
        if draft_layouts != "common":
            exif["draft_layouts"] = draft_layouts
        if decode == "device":
            blobs = []
            for p in paths:
                with open(p, "rb") as f:
                    blobs.append(f.read())
            return self.from_jpeg_bytes(blobs, draft=draft, regions=regions, non_rgb=non_rgb, **exif)
        if decode != "host":
            raise ValueError(f"decode must be 'host' or 'device', not {decode!r}")
        exif.pop("cmyk", None)
        exif.pop("layouts", None)
        exif.pop("draft_layouts", None)
        arrays = [self._pil_rgb(Image.open(p), (self.S, self.S) if draft else None, non_rgb, **exif) for p in paths]
        if regions is None:
            return self(arrays)
        for a in arrays:
            self._check_size(a.shape[0], a.shape[1])
        return self.resize_regions([torch.from_numpy(a.copy()).to(self.device) for a in arrays], regions)

    @staticmethod
    def _pil_rgb(pil, draft=None, non_rgb="black", orientation="ignore") -> np.ndarray:
        """The host decode of one opened file: the draft request if there is one, then for non-RGB modes a black canvas
        (of the size the draft left) or, with non_rgb="convert", PIL's `convert("RGB")`, then with orientation="exif"
        the transposition `ImageOps.exif_transpose` picks for the file → uint8 (H,W,3) array."""
        if draft is not None:
            pil.draft("RGB", draft)
        turn = 1
        if orientation != "ignore":
            from .jpeg import pil_orientation
            turn = pil_orientation(pil)                                  # of the file: a converted image may lose its tag
        if pil.mode != "RGB":
            pil = pil.convert("RGB") if non_rgb == "convert" else Image.new("RGB", pil.size)
        if turn != 1:
            from .jpeg import transpose_method
            pil = pil.transpose(transpose_method(turn))
        return np.asarray(pil, dtype=np.uint8)

    # ---------------------------------------------------------------------------------------------------------
    # device JPEG decode
    # ---------------------------------------------------------------------------------------------------------
    def _host_rgb(self, blob, draft=None, non_rgb="black", orientation="ignore") -> np.ndarray:
        """The host path for one file: PIL decode, after `im.draft("RGB", draft)` if there is a draft request (black
        canvas for non-RGB modes, of the drafted size, or their `convert("RGB")`), turned upright with
        orientation="exif" → uint8 (H,W,3) array."""
        return self._pil_rgb(Image.open(io.BytesIO(blob)), draft, non_rgb, orientation)

    @staticmethod
    def _grow(buf, nbytes, **kw):
        if buf is not None and buf.numel() >= nbytes:
            return buf
        return torch.empty(max(nbytes, 2 * (buf.numel() if buf is not None else 0)), dtype=torch.uint8, **kw)

    @staticmethod
    def _set_fields(struct, totals):
        for k, v in totals.items():
            if isinstance(v, list):
                getattr(struct, k)[:len(v)] = v
            else:
                setattr(struct, k, v)

    @property
    def last_routes(self):
        """How each file of the last `decode_jpeg` / `from_jpeg_bytes` call was decoded, in input order: "device" (baseline,
        odic_jpeg_decode), "device-progressive" (odic_jpeg_decode_progressive), "device-cmyk" (four components,
        odic_jpeg_any_decode), "device-layout" (three components at a layout of layouts="all", the same call),
        "device-progressive-cmyk" / "device-progressive-layout" (the progressive files of those two kinds,
        odic_jpeg_decode_progressive_any), "host"
        (PIL: a kind the device does not
        take), "host-after-status" (the device reported status 1 and PIL decoded the file again) or "black"."""
        return tuple(self._jpeg_routes)

    @property
    def last_orientations(self):
        """The EXIF orientation applied to each file of the last `decode_jpeg` / `from_jpeg_bytes` call, in input order:
        2..8, or 1 for none (no tag, a value Pillow does not transpose by, or orientation="ignore")."""
        return tuple(self._jpeg_orientations)

    def decode_jpeg(self, blobs, subseq_bits: int = 2048, max_sync_passes: int = 4, progressive: str = "host",
                    draft=None, non_rgb: str = "black", orientation: str = "ignore", cmyk: str = "host",
                    layouts: str = "common", draft_layouts: str = "common"):
        """Compressed files (bytes) → list of uint8 (H,W,3) RGB tensors on the device, each equal to
        np.asarray(PIL.Image.open(f)) (an all-black canvas for non-RGB files, as the host path; with
        non_rgb="convert" each equals np.asarray(PIL.Image.open(f).convert("RGB")) instead: one-component JPEGs take the
        device routes below like three-component ones, four-component JPEGs and every other non-RGB file go to PIL, and
        no route is "black").  Baseline JPEGs are
        decoded by odic_jpeg_decode and, with progressive="device", progressive ones by odic_jpeg_decode_progressive
        (the default "host" sends them to PIL until the device route is measured faster), each kind in one batched call, with one host-to-device copy and one status read-back
        for both; the rest, and images the device rejects, by PIL.  Exceptions are the host path's, in its order: PIL's,
        file by file, then the size check of `__call__`.  Ordered after the work on the CURRENT stream.
        draft=(width, height): every file is decoded as after `im.draft("RGB", draft)`, at 1/2, 1/4 or 1/8 of its size
        while both sides stay at least the requested ones (`jpeg.draft_scale`), by odic_jpeg_decode_scaled /
        odic_jpeg_decode_progressive_scaled or by PIL with the same request; sizes, black canvases and the size check
        are those of the drafted image.
        orientation="exif": every image is returned upright, equal to `np.asarray(ImageOps.exif_transpose(im))` of the
        image the rules above describe (after the draft and the non-RGB rule: a black canvas has the transposed size),
        in the oriented shape.  Files decoded on the device are permuted there by one odic_orient_rgb8 launch into one
        new buffer, files PIL decodes by PIL; the routes are the same as without it.  `last_orientations` reports the
        value applied to each file (`jpeg.exif_orientation`).
        cmyk="device" (needs non_rgb="convert"; the default "host" leaves them to PIL until the device route is
        measured): baseline four-component JPEGs — CMYK, or YCCK by Adobe transform 2 — that
        `jpeg.parse` admits are decoded by one odic_jpeg_any_decode call in the same upload and status read-back, route
        "device-cmyk", each equal to np.asarray(PIL.Image.open(f).convert("RGB")).  Progressive four-component files
        stay with PIL unless progressive="device" is given too (below), and so do all of them under a draft request
        unless draft_layouts="all" (below).
        layouts="all" (the default "common" leaves them to PIL until the device route is measured):
        baseline three-component JPEGs that only `jpeg.parse(f, layouts="all")` admits — luma at 1x2 (4:4:0), 4x1
        (4:1:1), 4x2 (4:1:0), chroma sub-sampled one way under a 2x2 luma, a component 0 that is not the largest, files
        stored as RGB — are decoded by that odic_jpeg_any_decode call too (one call for both kinds), route
        "device-layout", each equal to np.asarray(PIL.Image.open(f).convert("RGB")).  A file the common rules admit keeps
        its route.  Progressive files with these layouts stay with PIL unless progressive="device" is given too, and
        so do all of them under a draft request unless draft_layouts="all".
        progressive="device" together with cmyk="device", or together with layouts="all" (both opt-ins; any other
        combination of keywords does exactly what it did): the progressive files of that kind — SOF2 frames of four
        components, or of three at a layout only layouts="all" admits — that `jpeg.parse_progressive(f, non_rgb,
        cmyk=, layouts=)` admits are decoded by one odic_jpeg_decode_progressive_any call in the same upload and
        status read-back, routes "device-progressive-cmyk" / "device-progressive-layout" (DESIGN §4.27), each equal to
        np.asarray(PIL.Image.open(f).convert("RGB")).  Under a draft request they stay with PIL, as their baseline
        siblings do, unless draft_layouts="all".
        draft_layouts="all" (the default "common" withholds cmyk= and layouts= from the parsers under a draft request,
        so that their files go to PIL with the same request): the files those two keywords admit keep their four routes
        under a draft and are decoded at the draft scale by odic_jpeg_any_decode_scaled and
        odic_jpeg_decode_progressive_any_scaled, every component at libjpeg's own transform size for that scale
        (`jpeg.scaled_components`), each equal to what PIL makes of the file after `im.draft("RGB", draft)`
        and `convert("RGB")`.  Without a draft request it changes nothing."""
        from . import jpeg as J
        if progressive not in ("device", "host"):
            raise ValueError(f"progressive must be 'device' or 'host', not {progressive!r}")
        J.check_non_rgb(non_rgb)
        J.check_orientation(orientation)
        J.check_cmyk(cmyk, non_rgb)
        opt = () if non_rgb == "black" else (non_rgb,)                   # the default's calls stay as they are
        J.check_layouts(layouts)
        J.check_draft_layouts(draft_layouts)
        if draft is not None:
            draft = (int(draft[0]), int(draft[1]))
            if draft[0] <= 0 or draft[1] <= 0:
                raise ValueError(f"draft wants a positive (width, height), not {draft!r}")
        blobs = [bytes(b) for b in blobs]
        rp = J.plan_routes(blobs, progressive, draft, non_rgb, cmyk, layouts, draft_layouts, self.max_bytes)
        hdrs, scales, sizes, routes = rp.hdrs, rp.scales, rp.sizes, rp.routes
        order = rp.order
        exif = orientation != "ignore"
        turns = [J.header_orientation(h, b) if exif else 1 for h, b in zip(hdrs, blobs)]
        host_kw = {"orientation": orientation} if exif else {}           # the default's calls stay as they are
        out = [None] * len(blobs)
        if order:
            groups = [(kind, [hdrs[i] for i in idx], [blobs[i] for i in idx]) for kind, idx in rp.groups]
            status, rgb, out_offs = self._decode_on_device(groups, subseq_bits, max_sync_passes,
                                                           [scales[i] for i in order])
            turned = []                                                  # (image, its offset in rgb): to be permuted
            for k, i in enumerate(order):
                if status[k] != 0:
                    routes[i] = "host-after-status"
                elif turns[i] != 1:
                    turned.append((i, out_offs[k]))
                else:
                    w, h = sizes[i]
                    out[i] = rgb[out_offs[k]:out_offs[k] + w * h * 3].view(h, w, 3)
            if turned:
                self._orient_on_device(rgb, turned, sizes, turns, out)
        self._jpeg_routes, self._jpeg_orientations = routes, turns
        for i, h in enumerate(hdrs):                                     # input order, as the host path
            if h.kind != J.BLACK and out[i] is None:
                out[i] = self._host_rgb(blobs[i], draft, *opt, **host_kw)
        for i, h in enumerate(hdrs):
            if h.kind == J.BLACK:
                w, hh = J.oriented_size(sizes[i], turns[i])
                self._check_size(hh, w)
                out[i] = torch.zeros(hh, w, 3, dtype=torch.uint8, device=self.device)
            else:
                self._check_size(out[i].shape[0], out[i].shape[1])
                if isinstance(out[i], np.ndarray):
                    out[i] = torch.from_numpy(out[i].copy()).to(self.device)
        return out

    def _orient_on_device(self, rgb, turned, sizes, turns, out) -> None:
        """One odic_orient_rgb8 call on self.stream, behind the decode launches: the images `turned` [(index, byte offset
        in rgb)] of (width, height) sizes[index], from the shared decode buffer into one new buffer, 256-aligned slots;
        out[index] becomes the oriented (H,W,3) view."""
        from .jpeg import oriented_size
        rec = np.zeros(len(turned), ORIENT_JOB_DTYPE)
        pos = 0
        for r, (i, off) in zip(rec, turned):
            w, h = sizes[i]
            r["src_off"], r["dst_off"], r["src_stride_bytes"] = off, pos, 3 * w
            r["H"], r["W"], r["orientation"] = h, w, turns[i]
            pos += _pad256(w * h * 3)
        dst = torch.empty(pos, dtype=torch.uint8, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        self._hip.check(self.lib.odic_orient_rgb8(rec.ctypes.data, len(rec), rgb.data_ptr(), dst.data_ptr(),
                                                  self.stream.cuda_stream), "odic_orient_rgb8")
        torch.cuda.current_stream().wait_stream(self.stream)
        for r, (i, _) in zip(rec, turned):
            w, h = oriented_size(sizes[i], turns[i])
            out[i] = dst[int(r["dst_off"]):int(r["dst_off"]) + w * h * 3].view(h, w, 3)

    #: group kind (jpeg.GROUP_KINDS) → (batch struct of _hip, workspace query, entry point; `_scaled` for a draft scale)
    _JPEG_CALLS = {
        "base": ("JpegBatch", "odic_jpeg_workspace_bytes", "odic_jpeg_decode"),
        "prog": ("JpegProgBatch", "odic_jpeg_progressive_workspace_bytes", "odic_jpeg_decode_progressive"),
        "own": ("JpegBatch", "odic_jpeg_any_workspace_bytes", "odic_jpeg_any_decode"),
        "pany": ("JpegProgBatch", "odic_jpeg_progressive_any_workspace_bytes", "odic_jpeg_decode_progressive_any"),
    }

    def _decode_on_device(self, groups, subseq_bits, max_sync_passes, scales):
        """One decode call per group of `groups` ([(kind, headers, files)] as `jpeg.plan_device_batch` takes them):
        odic_jpeg_decode, odic_jpeg_decode_progressive, odic_jpeg_any_decode or odic_jpeg_decode_progressive_any
        (`_JPEG_CALLS`), sharing one upload, one output buffer, one workspace and one status read-back → (status numpy
        int32 in group order, uint8 RGB buffer, byte offset per image).  scales: the draft scale of every image in group
        order; a group with a scale above 1 goes through its _scaled entry point, with the scales uploaded beside the
        headers.  This is the GPU half: `jpeg.plan_device_batch` lays the upload and the output out."""
        from . import jpeg as J
        plan = J.plan_device_batch(groups, subseq_bits, scales)
        n_all = len(plan.out_offs)
        self._jpeg_ev.synchronize()                                      # the previous batch's upload is done
        self._jpeg_pinned = self._grow(self._jpeg_pinned, plan.total, pin_memory=True)
        self._jpeg_status = self._grow(self._jpeg_status, 4 * n_all, pin_memory=True)
        plan.fill(self._jpeg_pinned.numpy())
        rgb = torch.empty(max(plan.groups[-1].out_off + plan.groups[-1].out_bytes, 1), dtype=torch.uint8,
                          device=self.device)
        status = torch.empty(n_all, dtype=torch.int32, device=self.device)
        calls = []                                                       # (group, batch struct, workspace bytes, entry)
        for g in sorted(plan.groups, key=lambda g: g.kind == "prog"):    # "prog" last: its coefficients stay in the
            struct, query, entry = self._JPEG_CALLS[g.kind]              # workspace (`progressive_coefficients`)
            b = getattr(self._hip, struct)()
            b.n_images = g.n
            if struct == "JpegBatch":
                b.subseq_bits, b.max_sync_passes = subseq_bits, max_sync_passes
            self._set_fields(b, g.tot)
            need = getattr(self.lib, query)(ctypes.byref(b))
            if need == 0 and struct == "JpegProgBatch":
                raise RuntimeError("JPEG batch too large for one progressive decode call")
            calls.append((g, b, need, entry))
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            self._jpeg_dev = self._grow(self._jpeg_dev, plan.total, device=self.device)
            self._jpeg_ws = self._grow(self._jpeg_ws, max(need for _, _, need, _ in calls), device=self.device)
            self._jpeg_dev[:plan.total].copy_(self._jpeg_pinned[:plan.total], non_blocking=True)
            self._jpeg_ev.record(self.stream)
            base = self._jpeg_dev.data_ptr()
            for g, b, need, entry in calls:
                b.headers = base + g.offs[0]
                if len(g.offs) == 3:
                    b.scans, b.tables = base + g.offs[1], base + g.offs[2]
                b.data, b.out = base + plan.data_off, rgb.data_ptr() + g.out_off
                b.status = status.data_ptr() + 4 * g.first
                args = [ctypes.byref(b), self._jpeg_ws.data_ptr(), need, self.stream.cuda_stream]
                if any(s > 1 for s in scales[g.first:g.first + g.n]):
                    entry += "_scaled"
                    args.insert(1, base + plan.scale_off + 4 * g.first)
                self._hip.check(getattr(self.lib, entry)(*args), entry)
                if g.kind == "prog":
                    self._jpeg_prog_coef = (self.lib.odic_jpeg_progressive_coef_offset(ctypes.byref(b)), plan.coef_off)
            st = self._jpeg_status[:4 * n_all].view(torch.int32)
            st.copy_(status, non_blocking=True)
        self.stream.synchronize()                                        # the one host synchronisation
        torch.cuda.current_stream().wait_stream(self.stream)
        return st.numpy().copy(), rgb, plan.out_offs

    def progressive_coefficients(self, k: int) -> torch.Tensor:
        """Diagnostic: the int16 [blocks, 64] natural-order coefficients (MCU by MCU, DC as its value) of the k-th file
        routed "device-progressive" in the last call, read from the workspace; valid until the next call."""
        byte_off, blocks = self._jpeg_prog_coef
        lo, hi = byte_off + 128 * blocks[k], byte_off + 128 * blocks[k + 1]
        return self._jpeg_ws[lo:hi].view(torch.int16).view(-1, 64).clone()

    def from_jpeg_bytes(self, blobs, subseq_bits: int = 2048, max_sync_passes: int = 4,
                        progressive: str = "host", draft: bool = False, regions=None,
                        non_rgb: str = "black", orientation: str = "ignore", cmyk: str = "host",
                        layouts: str = "common", draft_layouts: str = "common") -> torch.Tensor:
        """Compressed files (bytes) → normalised fp32 [B,3,S,S]: `decode_jpeg` + the resize / normalise kernel,
        torch.equal to `from_files` on the same files (with the same `draft`: True requests (S, S) of `decode_jpeg`,
        the same `non_rgb` and the same `orientation`).
        regions: a sequence of (file index, (l, t, r, b)) → the region batch fp32 [N,3,S,S] of `resize_regions` on the
        decoded images instead; with draft=True the boxes are in the coordinates of the drafted image, with
        orientation="exif" in those of the upright one.  cmyk: as `decode_jpeg` (with draft=True four-component files
        stay on the host route unless draft_layouts="all"); layouts: as `decode_jpeg` (likewise); draft_layouts: as
        `decode_jpeg`."""
        exif = {} if orientation == "ignore" else {"orientation": orientation}   # the default's call stays as it is
        if cmyk != "host":
            exif["cmyk"] = cmyk
        if layouts != "common":
            exif["layouts"] = layouts
        if draft_layouts != "common":
            exif["draft_layouts"] = draft_layouts
        imgs = self.decode_jpeg(blobs, subseq_bits, max_sync_passes, progressive,
                                draft=(self.S, self.S) if draft else None, non_rgb=non_rgb, **exif)
        if regions is not None:
            return self.resize_regions(imgs, regions)
        S = self.S
        out = torch.empty(len(imgs), 3, S, S, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for i, img in enumerate(imgs):
                H, W, _ = img.shape
                self._check_size(H, W)
                self._jpeg_tmp = self._resize_whole(img.data_ptr(), H, W, self._jpeg_tmp, out[i])
        torch.cuda.current_stream().wait_stream(self.stream)
        return out

    # ---------------------------------------------------------------------------------------------------------
    # regions: PIL's resize(..., box=) for N boxes of images on the device, in one launch pair
    # ---------------------------------------------------------------------------------------------------------
    def resize_regions(self, images, regions) -> torch.Tensor:
        """images: list of uint8 (H,W,3) RGB tensors on the device, as `decode_jpeg` returns them (contiguous, or views
        into one buffer whose pixels are 3 contiguous bytes); regions: sequence of (image index, (l, t, r, b)) with float
        boxes in pixels → normalised fp32 [N,3,S,S] in region order, row n equal to
        `normalise(PIL.Image.resize((S, S), BILINEAR, box=box))` of its image (not crop-then-resize: the filter reads the
        pixels just outside the box, as Pillow's does).  One odic_resize_boxes_normalize call; images that do not share
        one storage are first copied into one buffer.  ValueError for an index or a box outside its image
        (0 <= l < r <= W, 0 <= t < b <= H).  Ordered after the work on the CURRENT stream."""
        S = self.S
        regions = [(int(i), tuple(box)) for i, box in regions]
        out = torch.empty(len(regions), 3, S, S, dtype=torch.float32, device=self.device)
        if not regions:
            return out
        used = sorted({i for i, _ in regions})
        if used[0] < 0 or used[-1] >= len(images):
            raise ValueError(f"region of image {used[0] if used[0] < 0 else used[-1]}: there are {len(images)} images")
        for i in used:
            im = images[i]
            if not (isinstance(im, torch.Tensor) and im.dtype == torch.uint8 and im.dim() == 3 and im.shape[2] == 3
                    and im.device == out.device and im.numel() > 0 and im.stride(2) == 1 and im.stride(1) == 3
                    and im.stride(0) >= 3 * im.shape[1]):
                raise RuntimeError(f"resize_regions wants uint8 (H,W,3) RGB tensors on {self.device} (image {i})")
        shared = len({images[i].untyped_storage().data_ptr() for i in used}) == 1
        if shared:
            src_base = min(images[i].data_ptr() for i in used)
            place = {i: (images[i].data_ptr() - src_base, images[i].stride(0)) for i in used}
        else:                                                            # one 256-aligned slot per image, rows packed
            place, pos = {}, 0
            for i in used:
                place[i] = (pos, 3 * images[i].shape[1])
                pos += _pad256(images[i].numel())
            gather_bytes = pos
        rec, bounds, coefs, tmp_bytes, max_rows = pack_resize_jobs(
            [(place[i][0], images[i].shape[0], images[i].shape[1], place[i][1], box) for i, box in regions], S)
        off_b = _pad256(rec.nbytes)
        off_k = off_b + _pad256(bounds.nbytes)
        tables = np.zeros(off_k + coefs.nbytes, np.uint8)
        for o, a in ((0, rec), (off_b, bounds), (off_k, coefs)):
            tables[o:o + a.nbytes] = np.frombuffer(a.tobytes(), np.uint8)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            if not shared:
                self._region_src = self._grow(self._region_src, gather_bytes, device=self.device)
                src_base = self._region_src.data_ptr()
                for i in used:
                    self._gather(images[i], self._region_src[place[i][0]:place[i][0] + images[i].numel()])
            self._region_tmp = self._grow(self._region_tmp, tmp_bytes, device=self.device)
            dev = torch.from_numpy(tables).to(self.device)
            self._hip.check(self.lib.odic_resize_boxes_normalize(
                dev.data_ptr(), len(regions), src_base, dev.data_ptr() + off_b, dev.data_ptr() + off_k,
                self._region_tmp.data_ptr(), tmp_bytes, out.data_ptr(), S, max_rows, self._mean, self._std,
                self.stream.cuda_stream), "odic_resize_boxes_normalize")
        torch.cuda.current_stream().wait_stream(self.stream)
        return out

    def _gather(self, img: torch.Tensor, dst: torch.Tensor) -> None:
        """img (H,W,3) → the flat uint8 `dst` of as many bytes, on self.stream: odic_copy for the whole 16-byte words of a
        contiguous, 16-byte aligned image (dst slots are 256-aligned), a strided copy for its last bytes or for a view
        with a row pitch."""
        n = img.numel()
        n16 = n & ~15 if img.is_contiguous() and img.data_ptr() % 16 == 0 else 0
        if n16:
            self._hip.check(self.lib.odic_copy(img.data_ptr(), dst.data_ptr(), n16, self.stream.cuda_stream), "odic_copy")
        if n16 < n:
            if n16:
                dst[n16:].copy_(img.view(-1)[n16:])
            else:
                dst.view(img.shape).copy_(img)
