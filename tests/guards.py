"""Guarded buffers for containment tests: an operand that lives INSIDE one larger live allocation whose every other byte is
poison, so that a kernel writing (or reading) outside its operand changes a byte (or produces a NaN) instead of faulting.

Layout of one allocation (flat uint8):

    [ front band | batch 0: rows x ld | gap | batch 1: rows x ld | gap | ... | last batch: rows x ld | back band ]

with `stride` elements from one batch to the next (gap = stride - rows·ld) and, inside every row, the operand's `cols`
elements followed by ld - cols padding elements.  Everything that is not operand data holds the byte 0xFF: a NaN in fp32,
bf16, fp16, fp8-e4m3fn and in both halves of a split-fp16 pair, -1 in the integer types.  One pattern serves both
directions: a stray write of anything else shows up as a changed byte, a stray read of it turns the result into NaN.

Each band is one tile of the tallest GEMM tile configuration (TALLEST_TILE_ROWS rows of `ld` elements; the tile tables of
csrc/gemm_bf16.hip, gemm_x3.hip and gemm_lowp.hip — tests/test_guards.py re-derives the number from those files) and never
less than 4 KiB: a kernel that stores or fetches a whole tile where the operand ends stays inside the allocation.

Not a conftest: import it (`import guards`), like test_jpeg_gpu.py imports test_jpeg_host.
"""
from __future__ import annotations

import numpy as np
import torch

POISON = 0xFF
TALLEST_TILE_ROWS = 288          # bf16 tile_cfg 40 / split-fp16 tile_cfg 6: 6 waves x 3 x 16 rows
MIN_BAND_BYTES = 4096
_ALIGN = 256                     # the operand starts as aligned as a fresh torch allocation

#: dtype marker of split-fp16 ("h2") tensors.  They travel as torch.int32 of the logical shape (ops.H2_DTYPE), but inside
#: a row every 8 elements are 32 bytes [8 x fp16 hi | 8 x fp16 lo]: element c does NOT own bytes 4c..4c+3.
H2 = "h2"


def _torch_dtype(dtype):
    return torch.int32 if dtype == H2 else dtype


def _esize(dtype) -> int:
    return torch.empty(0, dtype=_torch_dtype(dtype)).element_size()


def owned_bytes(cols: int, ld: int, dtype) -> np.ndarray:
    """Boolean mask over the ld·esize bytes of one row: True where the byte belongs to one of the first `cols` elements."""
    es = _esize(dtype)
    m = np.zeros(ld * es, dtype=bool)
    if dtype == H2:
        if ld % 8:
            raise ValueError("split-fp16 rows are whole groups of 8 elements (ld % 8 == 0)")
        c = np.arange(cols)
        hi = (c // 8) * 32 + (c % 8) * 2
        for off in (0, 1, 16, 17):
            m[hi + off] = True
    else:
        m[:cols * es] = True
    return m


def band_bytes(ld: int, dtype) -> int:
    n = max(MIN_BAND_BYTES, TALLEST_TILE_ROWS * ld * _esize(dtype))
    return -(-n // _ALIGN) * _ALIGN


class Guarded:
    def __init__(self, rows, cols, ld, dtype, device, batch=1, stride=None):
        if ld < cols or rows <= 0 or cols <= 0 or batch <= 0:
            raise ValueError("need rows, cols, batch > 0 and ld >= cols")
        stride = rows * ld if stride is None else stride
        if batch > 1 and stride < rows * ld:
            raise ValueError("stride < rows * ld: batches would overlap")
        if dtype == H2 and ld % 8:
            raise ValueError("split-fp16 rows are whole groups of 8 elements (ld % 8 == 0)")
        self.rows, self.cols, self.ld, self.dtype, self.batch, self.stride = rows, cols, ld, dtype, batch, stride
        self.es = _esize(dtype)
        self.band = band_bytes(ld, dtype)
        self.body_elems = (batch - 1) * stride + rows * ld
        self.body_bytes = self.body_elems * self.es
        self.raw = torch.full((2 * self.band + self.body_bytes,), POISON, dtype=torch.uint8, device=device)
        body = self.raw[self.band:self.band + self.body_bytes].view(_torch_dtype(dtype))
        self.t = torch.as_strided(body, (batch, rows, ld), (stride, ld, 1))
        if batch == 1:
            self.t = self.t[0]

    # -- views ---------------------------------------------------------------------------------------------------------
    @property
    def t3(self) -> torch.Tensor:
        return self.t if self.batch > 1 else self.t[None]

    def data_ptr(self) -> int:
        return self.t.data_ptr()

    def fill_data(self, data: torch.Tensor) -> "Guarded":
        """Write real data into the operand region [batch, rows, cols]; padding, gaps and bands keep their poison."""
        if self.dtype == H2 and self.cols % 8:
            raise ValueError("split-fp16 data is copied in whole groups of 8 elements")
        src = data.reshape(self.batch, self.rows, self.cols).to(self.raw.device)
        if src.dtype != _torch_dtype(self.dtype):
            raise ValueError(f"data is {src.dtype}, buffer is {self.dtype}")
        # (through integer views: a float copy could canonicalise NaN payloads)
        it = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.es]
        self.t3.view(it)[:, :, :self.cols].copy_(src.contiguous().view(it))
        return self

    def _rows_u8(self) -> np.ndarray:
        """CPU bytes of the body as [batch, rows, ld·es] (a copy)."""
        body = self.raw[self.band:self.band + self.body_bytes].cpu().numpy()
        sb, rb = self.stride * self.es, self.ld * self.es
        return np.lib.stride_tricks.as_strided(body, (self.batch, self.rows, rb), (sb, rb, 1))

    def data_bytes(self, cols=None) -> torch.Tensor:
        """The operand's own bytes, [batch, rows, n] uint8 on the CPU — equal between two layouts of the same values."""
        m = owned_bytes(self.cols if cols is None else cols, self.ld, self.dtype)
        return torch.from_numpy(np.ascontiguousarray(self._rows_u8()[:, :, m]))

    def values(self, cols=None) -> torch.Tensor:
        """The operand as float64 [batch, rows, cols] on the CPU (split fp16: hi + lo); `cols` up to ld decodes the padding too."""
        cols = self.cols if cols is None else cols
        if self.dtype == H2:
            g = torch.from_numpy(np.ascontiguousarray(self._rows_u8())).view(torch.float16)
            g = g.reshape(self.batch, self.rows, self.ld // 8, 2, 8).double()
            return (g[..., 0, :] + g[..., 1, :]).reshape(self.batch, self.rows, self.ld)[..., :cols]
        v = self.t3[:, :, :cols].cpu()
        return v.double() if v.dtype.is_floating_point else v.to(torch.float64)

    # -- the check -----------------------------------------------------------------------------------------------------
    def assert_untouched(self, written_cols=None, what: str = "") -> None:
        """Bitwise: front band, back band, columns [written_cols, ld) of every row and the gaps between batches still hold
        the poison byte.  Reports region, batch, row, column (element index inside the row) and the byte found."""
        wc = self.cols if written_cols is None else written_cols
        raw = self.raw.cpu().numpy()
        tag = f"{what}: " if what else ""

        def fail(region, b, r, c, off, byte):
            raise AssertionError(f"{tag}stray write in {region}: batch {b}, row {r}, column {c}, byte offset {off} of the "
                                 f"allocation holds 0x{int(byte):02X}, expected 0x{POISON:02X}")

        front = raw[:self.band]
        bad = np.flatnonzero(front != POISON)
        if bad.size:
            k = int(bad[-1])                       # the byte nearest to the operand
            back_elems = (self.band - k + self.es - 1) // self.es
            fail("front band", 0, -((back_elems + self.ld - 1) // self.ld), (-back_elems) % self.ld, k, front[k])
        back = raw[self.band + self.body_bytes:]
        bad = np.flatnonzero(back != POISON)
        if bad.size:
            k = int(bad[0])
            e = k // self.es
            fail("back band", self.batch - 1, self.rows + e // self.ld, e % self.ld, self.band + self.body_bytes + k, back[k])
        body = raw[self.band:self.band + self.body_bytes]
        sb, rb = self.stride * self.es, self.ld * self.es
        rows = np.lib.stride_tricks.as_strided(body, (self.batch, self.rows, rb), (sb, rb, 1))
        pad = ~owned_bytes(wc, self.ld, self.dtype)
        if pad.any():
            idx = np.flatnonzero(pad)
            hit = np.argwhere(rows[:, :, idx] != POISON)
            if hit.size:
                b, r, j = (int(v) for v in hit[0])
                o = int(idx[j])
                col = (o // 32) * 8 + (o % 16) // 2 if self.dtype == H2 else o // self.es
                fail("pad column", b, r, col, self.band + b * sb + r * rb + o, rows[b, r, o])
        if self.batch > 1 and self.stride > self.rows * self.ld:
            for b in range(self.batch - 1):
                lo, hi = b * sb + self.rows * rb, (b + 1) * sb
                bad = np.flatnonzero(body[lo:hi] != POISON)
                if bad.size:
                    k = int(bad[0])
                    e = k // self.es
                    fail("batch gap", b, self.rows + e // self.ld, e % self.ld, self.band + lo + k, body[lo + k])

    def assert_all_poison(self, what: str = "") -> None:
        """Nothing at all was written (a launch the header says changes nothing)."""
        bad = torch.nonzero(self.raw != POISON)
        assert bad.numel() == 0, f"{what}: byte {int(bad[0])} of the allocation was written"


def guarded(rows, cols, ld, dtype, device, batch=1, stride=None) -> Guarded:
    """An OUTPUT of `rows` x `cols` elements with leading dimension `ld` (and `batch` of them `stride` elements apart), all
    poison, inside a poisoned allocation.  `.t` is the [rows, ld] / [batch, rows, ld] view to hand to the kernel."""
    return Guarded(rows, cols, ld, dtype, device, batch, stride)


def poisoned_input(t: torch.Tensor, rows, cols, ld, batch=1, stride=None, device=None, dtype=None) -> Guarded:
    """The same layout for an INPUT: the real data `t` ([batch,] rows, cols) in the operand region, 0xFF in columns
    [cols, ld), in the rows behind `rows` (the back band), between batches and in front."""
    g = Guarded(rows, cols, ld, dtype if dtype is not None else t.dtype, device if device is not None else t.device,
                batch, stride)
    return g.fill_data(t)
