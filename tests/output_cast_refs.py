"""What a kernel of this library must write when it narrows an fp32 value to one of its four output formats — bf16, fp16,
OCP e4m3 ("fp8") and split fp16 ("h2") — stated three ways, shared by test_output_casts_host.py (no GPU: the three agree,
and a wrong cast is told apart) and test_output_casts_gpu.py (every store path of the HIP kernels against them, bitwise):

  * PATTERNS[fmt]: fp32 bit patterns at the places a conversion goes wrong — rounding ties above an even and above an odd
    kept significand with their one-ulp neighbours, the subnormal range of the format with its ties, the largest finite
    value, the values just past it, ±inf and NaNs;
  * ref_codes(fmt, x): the reference, from torch's CPU casts (`.to(bfloat16)`, `.to(float16)`,
    `.clamp(-448, 448).to(float8_e4m3fn)`, `ops.h2_from_f32`);
  * model_codes(fmt, bits): an independent model in integer arithmetic on the bit pattern alone (round to nearest even, no
    torch cast), which also evaluates the four MUTATIONS — casts that are wrong in one way each.

The contract (include/odic_hip.h, DESIGN.md "Output casts"): nearest-even everywhere; e4m3 saturates finite values past
the range and ±inf to ±448; h2 saturates to ±65504; bf16 and fp16 overflow to inf as IEEE and torch do; NaN stays NaN.

A "code" is the element's bits as a non-negative integer (int64 tensors): 16 bits for bf16 / fp16, 8 for e4m3, and for h2
a pair [..., 2] = (hi, lo) of fp16 codes.  Codes compare with `mismatch`: equal bits, or two zeros of either sign, or two
NaNs of any payload.

Not a conftest: import it (`import output_cast_refs as OC`), like frontend_refs.py.
"""
from __future__ import annotations

import struct
from typing import NamedTuple

import torch

from frontend_refs import CAST_FINITE_BITS, CAST_INF_BITS, CAST_NAN_BITS, _bits

FORMATS = ("bf16", "fp16", "e4m3", "h2")
CLASSES = ("tie-even", "tie-odd", "subnormal", "limit", "past-limit", "inf", "nan")


class Fmt(NamedTuple):
    mbits: int          # stored significand bits
    emin: int           # exponent of the smallest normal value
    max_q: int          # the largest finite value = max_q · 2^max_e, max_q < 2^(mbits + 1)
    max_e: int
    saturates: bool     # past the range: the largest finite value (True) or inf (False)

    @property
    def qmin(self):     # exponent of the last place in the subnormal range
        return self.emin - self.mbits


_FMT = {"bf16": Fmt(7, -126, 255, 120, False),      # 255 · 2^120 = 0x7F7F
        "fp16": Fmt(10, -14, 2047, 5, False),       # 2047 · 2^5 = 65504
        "e4m3": Fmt(3, -6, 14, 5, True)}            # 14 · 2^5 = 448 (the all-ones significand of the top binade is NaN)
_FMT["h2"] = _FMT["fp16"]._replace(saturates=True)  # (the hi half; classification only)


def f32_bits(v: float) -> int:
    return struct.unpack("<I", struct.pack("<f", v))[0]


def _both_signs(words):
    return [w ^ s for w in words for s in (0, 0x80000000)]


def _with_neighbours(words):
    return [w + d for w in words for d in (0, 1, -1)]


#: bf16: the shared list has ties (even, odd, neighbours), subnormals, values past the range, ±inf and NaNs; the two values
#: that must come out as the LARGEST FINITE bf16 (itself, and the last fp32 under the tie to inf) are added so that the
#: list has every class, and two ties in the subnormal range (to 0, and above an odd subnormal)
_BF16_EXTRA = _both_signs([0x7F7F0000, 0x7F7F7FFF, 0x00008000, 0x00018000])
#: e4m3 (3 stored bits; ulp 1/8 in [1, 2), 2 in [16, 32); subnormals k · 2^-9, k = 1..7)
_E4M3_EXTRA = _both_signs(
    [f32_bits(v) for v in (448.0, 464.0, 465.0, 1e9)] + [0x7F800000] +           # limit; the tie 448 | (480); past it; inf
    [f32_bits(464.0) - 1, f32_bits(448.0) + 1, f32_bits(432.0), f32_bits(416.0)] +     # under the tie; 432 = tie 416 | 448 (odd -> 448)
    _with_neighbours([f32_bits(v) for v in (1.0625, 1.1875, 17.0, 19.0)]) +     # ties above even / odd, two binades
    [f32_bits(2.0 ** -9), f32_bits(2.0 ** -10), f32_bits(2.0 ** -10) + 1, f32_bits(2.0 ** -10) - 1] +   # smallest subnormal; tie to 0
    [f32_bits(1.5 * 2.0 ** -9), f32_bits(2.5 * 2.0 ** -9)] +                    # subnormal ties above odd / even
    [f32_bits(7 * 2.0 ** -9)] + _with_neighbours([f32_bits(7.5 * 2.0 ** -9)]) + [f32_bits(2.0 ** -6)])  # largest subnormal | 2^-6
#: fp16 (10 stored bits: the low 13 bits of an fp32 significand go; subnormals k · 2^-24)
_FP16_EXTRA = _both_signs(
    [f32_bits(65504.0), f32_bits(65520.0) - 1, f32_bits(65520.0), f32_bits(65520.0) + 1, f32_bits(1e9)] +   # limit; 65519.996; the tie to inf
    _with_neighbours([0x3F801000, 0x3F803000, 0x42001000, 0x42003000]) +        # ties above even / odd, two binades
    [f32_bits(2.0 ** -24), f32_bits(2.0 ** -25), f32_bits(2.0 ** -25) + 1, f32_bits(2.0 ** -25) - 1] +
    [f32_bits(1.5 * 2.0 ** -24), f32_bits(2.5 * 2.0 ** -24)] +                  # subnormal ties above odd / even
    [f32_bits(1023 * 2.0 ** -24)] + _with_neighbours([f32_bits(1023.5 * 2.0 ** -24)]))  # largest subnormal, its tie to 2^-14


def _unique(words):
    return list(dict.fromkeys(words))


_BASE = CAST_FINITE_BITS + CAST_INF_BITS + CAST_NAN_BITS
PATTERNS = {"bf16": _unique(_BASE + _BF16_EXTRA),
            "fp16": _unique(_BASE + _FP16_EXTRA),
            "e4m3": _unique(_BASE + _E4M3_EXTRA)}
PATTERNS["h2"] = PATTERNS["fp16"]


def is_nan_bits(w: int) -> bool:
    return (w & 0x7F800000) == 0x7F800000 and (w & 0x007FFFFF) != 0


def values(words) -> torch.Tensor:
    """fp32 tensor with exactly these bit patterns (built through an integer view: NaN payloads survive)."""
    return _bits(list(words))


def take(fmt: str, idx: torch.Tensor, nan: bool = True) -> torch.Tensor:
    """fp32 of idx's shape: element = patterns[idx % P]; nan=False leaves the NaN patterns out of the list."""
    pats = values([w for w in PATTERNS[fmt] if nan or not is_nan_bits(w)]).view(torch.int32)
    return pats[idx % pats.numel()].view(torch.float32)


def rotated(fmt: str, n: int, r: int = 0, nan: bool = True) -> torch.Tensor:
    """[n] fp32: element i = patterns[(i + r) % P]."""
    return take(fmt, torch.arange(n) + r, nan)


# ====================================================================================================================
# codes and their comparison
# ====================================================================================================================
_NANMASK = {"bf16": (0x7F80, 0x007F), "fp16": (0x7C00, 0x03FF), "h2": (0x7C00, 0x03FF)}


def is_nan_code(fmt: str, c: torch.Tensor) -> torch.Tensor:
    """Per element (h2: per pair: the value hi + lo is NaN as soon as one half is)."""
    if fmt == "e4m3":
        return (c & 0x7F) == 0x7F
    em, mm = _NANMASK[fmt]
    n = ((c & em) == em) & ((c & mm) != 0)
    return n.any(-1) if fmt == "h2" else n


def _is_zero_code(fmt: str, c: torch.Tensor) -> torch.Tensor:
    return (c & (0x7F if fmt == "e4m3" else 0x7FFF)) == 0


def mismatch(fmt: str, got: torch.Tensor, want: torch.Tensor) -> torch.Tensor:
    """Boolean per element: the codes differ — except two zeros of either sign, and a NaN where a NaN is wanted."""
    assert got.shape == want.shape, (got.shape, want.shape)
    same = (got == want) | (_is_zero_code(fmt, got) & _is_zero_code(fmt, want))
    if fmt == "h2":
        same = same.all(-1)
    gn, wn = is_nan_code(fmt, got), is_nan_code(fmt, want)
    return torch.where(wn | gn, wn != gn, ~same)


def codes_of(fmt: str, t: torch.Tensor) -> torch.Tensor:
    """Codes of a CPU tensor in the format's storage type (bf16 / fp16 / float8_e4m3fn; h2: int32 [..., K], K % 8 == 0, each
    32 bytes = 8 hi halves then 8 lo halves) -> int64 [...] (h2: [..., K, 2])."""
    t = t.contiguous()
    if fmt == "e4m3":
        return t.view(torch.uint8).to(torch.int64)
    if fmt == "h2":
        g = t.view(torch.int16).reshape(*t.shape[:-1], -1, 2, 8).to(torch.int64) & 0xFFFF
        return torch.stack([g[..., 0, :], g[..., 1, :]], -1).reshape(*t.shape, 2)
    return t.view(torch.int16).to(torch.int64) & 0xFFFF


def ref_codes(fmt: str, x: torch.Tensor) -> torch.Tensor:
    """The reference: torch's CPU cast of fp32 `x` [..., n] to the format."""
    x = x.detach().cpu().float()
    if fmt == "bf16":
        return codes_of(fmt, x.to(torch.bfloat16))
    if fmt == "fp16":
        return codes_of(fmt, x.to(torch.float16))
    if fmt == "e4m3":
        return codes_of(fmt, x.clamp(-448.0, 448.0).to(torch.float8_e4m3fn))
    from on_device_image_captioning_amd import ops
    n = x.shape[-1]
    pad = torch.zeros(*x.shape[:-1], -(-n // 8) * 8)
    pad.view(torch.int32)[..., :n] = x.contiguous().view(torch.int32)
    return codes_of(fmt, ops.h2_from_f32(pad))[..., :n, :]


# ====================================================================================================================
# the integer model
# ====================================================================================================================
MUTATIONS = {                      # name -> (keyword arguments of model_codes, the formats it changes)
    "truncation": (dict(mode="trunc"), FORMATS),
    "round-half-up": (dict(mode="half-up"), FORMATS),
    "no saturation": (dict(saturate=False), ("e4m3", "h2")),
    "NaN -> -limit": (dict(nan_to_neg_limit=True), ("e4m3", "h2")),
}


def _decompose(w: int):
    """fp32 bits -> (sign, 'nan' | 'inf' | None, m, e): a finite value is m · 2^e, m an integer below 2^24."""
    s, e, f = w >> 31, (w >> 23) & 0xFF, w & 0x7FFFFF
    if e == 255:
        return s, ("nan" if f else "inf"), 0, 0
    return (s, None, f, -149) if e == 0 else (s, None, f | 0x800000, e - 150)


def _round(m: int, e: int, f: Fmt, mode: str = "rne"):
    """m · 2^e (m > 0) -> (q, qe, tie, odd): the nearest q · 2^qe with q < 2^(mbits + 1) and qe >= qmin, by `mode`; `tie`:
    the value lay exactly between two neighbours, `odd`: the lower of them had an odd last place."""
    p = f.mbits + 1
    qe = max(e + m.bit_length() - p, f.qmin)
    sh = qe - e
    if sh <= 0:
        return m << -sh, qe, False, False
    q, rem, half = m >> sh, m & ((1 << sh) - 1), 1 << (sh - 1)
    tie, odd = rem == half, bool(q & 1)
    if mode == "rne":
        up = rem > half or (tie and odd)
    elif mode == "half-up":
        up = rem >= half
    else:
        assert mode == "trunc"
        up = False
    q += up
    if q == 1 << p:
        q, qe = q >> 1, qe + 1
    return q, qe, tie, odd


def _past(q: int, qe: int, f: Fmt) -> bool:
    """q · 2^qe > the largest finite value."""
    sh = qe - f.max_e
    return (q << sh) > f.max_q if sh >= 0 else q > (f.max_q << -sh)


def _encode(s: int, q: int, qe: int, f: Fmt) -> int:
    width = {7: 16, 10: 16, 3: 8}[f.mbits]
    sign = s << (width - 1)
    if q < (1 << f.mbits):                       # zero or subnormal (then qe == qmin)
        return sign | q
    return sign | ((qe - f.qmin + 1) << f.mbits) | (q - (1 << f.mbits))


def _ieee16(w: int, f: Fmt, mode: str) -> int:
    """bf16 / fp16 of fp32 bits `w`: overflow -> inf, NaN -> a quiet NaN."""
    s, kind, m, e = _decompose(w)
    top = ((1 << (15 - f.mbits)) - 1) << f.mbits
    if kind == "nan":
        return (s << 15) | top | (1 << (f.mbits - 1))
    if kind == "inf":
        return (s << 15) | top
    if m == 0:
        return s << 15
    q, qe, _, _ = _round(m, e, f, mode)
    return (s << 15) | top if _past(q, qe, f) else _encode(s, q, qe, f)


def _e4m3(w: int, mode: str, saturate: bool, nan_to_neg_limit: bool) -> int:
    f = _FMT["e4m3"]
    s, kind, m, e = _decompose(w)
    if kind == "nan":
        return 0xFE if nan_to_neg_limit else (s << 7) | 0x7F
    if kind == "inf":
        return (s << 7) | (0x7E if saturate else 0x7F)        # (without the clamp the converter returns NaN past the range)
    if m == 0:
        return s << 7
    q, qe, _, _ = _round(m, e, f, mode)
    if _past(q, qe, f):
        return (s << 7) | (0x7E if saturate else 0x7F)
    return _encode(s, q, qe, f)


def _h2(w: int, mode: str, saturate: bool, nan_to_neg_limit: bool):
    """(hi, lo): hi = fp16(x clamped to ±65504), lo = fp16(x - hi); the difference is exact in integers."""
    f = _FMT["fp16"]
    s, kind, m, e = _decompose(w)
    if kind == "nan":
        return (0xFBFF, 0) if nan_to_neg_limit else ((s << 15) | 0x7E00, 0x7E00)
    if kind == "inf" or _past(m, e, f):
        if saturate:
            return (s << 15) | 0x7BFF, 0
        if kind == "inf" or _ieee16(w, f, mode) & 0x7FFF == 0x7C00:
            return (s << 15) | 0x7C00, 0x7E00                 # inf - inf = NaN
    if m == 0:
        return s << 15, 0
    q, qe, _, _ = _round(m, e, f, mode)
    hi = _encode(s, q, qe, f)
    sh = qe - e                                               # x - hi = (m - q·2^sh) · 2^e
    r = m - (q << sh) if sh >= 0 else 0
    if r == 0:
        return hi, 0
    rs = s ^ (r < 0)
    q2, qe2, _, _ = _round(abs(r), e, f, mode)
    return hi, _encode(rs, q2, qe2, f)


def model_codes(fmt: str, words, mode: str = "rne", saturate: bool = True, nan_to_neg_limit: bool = False) -> torch.Tensor:
    """Codes of the fp32 bit patterns `words` by integer arithmetic.  The defaults are the contract; the other arguments
    evaluate a wrong cast (MUTATIONS).  `saturate` and `nan_to_neg_limit` mean something for e4m3 and h2 only."""
    if fmt in ("bf16", "fp16"):
        return torch.tensor([_ieee16(w, _FMT[fmt], mode) for w in words], dtype=torch.int64)
    if fmt == "e4m3":
        return torch.tensor([_e4m3(w, mode, saturate, nan_to_neg_limit) for w in words], dtype=torch.int64)
    return torch.tensor([_h2(w, mode, saturate, nan_to_neg_limit) for w in words], dtype=torch.int64)


def classify(fmt: str, w: int) -> set:
    """The classes of CLASSES that the fp32 bit pattern `w` belongs to for this format (h2: for its hi half), by integer
    arithmetic: a tie counts inside the finite range only, `limit` is a value that must come out as the largest finite one,
    `past-limit` a finite value that cannot be represented (inf for bf16 / fp16, saturation for e4m3 / h2)."""
    f = _FMT[fmt]
    s, kind, m, e = _decompose(w)
    if kind:
        return {kind}
    if m == 0:
        return set()
    out = set()
    q, qe, tie, odd = _round(m, e, f)
    if _past(m, e, f) and (f.saturates or _past(q, qe, f)):
        return {"past-limit"}
    if (q, qe) == (f.max_q, f.max_e):
        out.add("limit")
    if tie:
        out.add("tie-odd" if odd else "tie-even")
    if e + m.bit_length() - 1 < f.emin:
        out.add("subnormal")
    return out
