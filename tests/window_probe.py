"""Probe harness for the window-attention kernels: every query-key pair's probability, one at a time.

An output element of window attention is a softmax-weighted mean over the N = ws² keys of a window, so a wrong bias entry
or mask bit for ONE key moves one weight out of N and can hide under a max-error bound.  The probe removes the mean: with a
one-hot V the output columns ARE the probabilities.

  * One-hot V.  In launch r, head h carries key chunk c = (h + r) % nchunk (nchunk = ceil(N / 32)):
    v[slot j, col d] = 1 iff j // 32 == c and j % 32 == d, so out[query i, head h, col d] = P[i, 32c + d].  With
    heads >= nchunk, nchunk launches return the whole P[b, window, head, query, key].  0 and 1 are exact in every dtype.
  * Rows are placed through oracle.expansionnet_ref.window_token_index: the harness works in (window, slot) order and the
    kernel's roll / partition / reverse map has to agree with the oracle's for the pairs to land where they belong.
  * Reference: softmax(scale·q·kᵀ + table[relative_position_index] + mask) in fp64, mask from
    weights.shifted_window_attn_mask (additive -100, as the reference model has it).
  * Four input families, all of values exact in bf16 AND fp16 (input rounding is not part of the comparison):
      bias    q = 0, table = per-head random permutation of linspace(-3, 3, (2ws-1)²): scores are bias + mask only, and
              neighbouring table entries differ widely;
      score   table = 0, k_j = code(j) (a random ±1 vector per slot), q_i = 2·code(i): scale·q·k = 0.25·<code_i, code_j>;
      peaked  both, q_i = 8·code(i): scores span ±32 plus the bias.  The codes come in pairs (slots j and N-1-j share one),
              so that a query has a second key at the row's top raw score, which on a seam window is usually masked;
      mask    q_i = 8·e_0, k_j = h(region(j))·e_0, h in {0, 40, 80} (MASK_H), table = 0: a masked key can sit only 20
              below the row maximum, P about 2e-9.  A kernel that took the mask for -inf would return 0 there.
  * Comparison: EVERY pair, |P_got − P_want| <= rtol·P_want + atol, with (rtol, atol) from the rounding steps of the output
    format (BOUNDS), never from a kernel's output.

Plain torch on the CPU; the GPU tests pass a callable that runs one launch.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Callable, Dict, NamedTuple, Optional, Tuple

import torch

from on_device_image_captioning_amd import weights as W
from oracle import expansionnet_ref as R

HD = 32                 # head dim of every kernel
HEADS = 6               # C = 192: >= nchunk = 5 of a 144-slot window
SCALE = 0.125           # exact; the kernels take any scale
FAMILIES = ("bias", "score", "peaked", "mask")

#: key height of the `mask` family per region id 3·ey + ex (edge class 0 / 1 / 2 = before the last window / last window
#: before the seam / behind the seam).  Regions that share a window differ in ex, in ey or in both between classes 1 and 2,
#: so 0 and 80 have to be one such step apart: 80 where exactly one axis is behind the seam, 40 where both are.  (Ids taken
#: mod 3 would not do: ids that share a window are {1, 2}, {3, 6} or {4, 5, 7, 8}, never 0 and 2 mod 3 together.)
MASK_H = (0.0, 0.0, 80.0, 0.0, 0.0, 80.0, 80.0, 80.0, 40.0)

#: (rtol, atol) per output format.  atol = the format's smallest step; rtol from its rounding steps:
#:   bf16  P is rounded to bf16 for the second MFMA and the output once more: 2 x 2^-8 < 1e-2;
#:   fp16  the same two roundings at 2^-11: 2e-3;
#:   fp32 / h2  no 16-bit rounding of P; what is left is the fp32 rounding of an exp argument of size |s| ~ 70
#:         (2^-17 absolute → 8e-6 relative) a few times over: 1e-4.
BOUNDS: Dict[str, Tuple[float, float]] = {
    "fp32": (1e-4, 1e-37),
    "bf16": (1e-2, 1e-37),
    "fp16": (2e-3, 2.0 ** -23),
    "h2": (1e-4, 2.0 ** -23),
}


@dataclass(frozen=True)
class Geometry:
    B: int
    res: int
    ws: int
    shift: int
    heads: int = HEADS

    @property
    def N(self) -> int:
        return self.ws * self.ws

    @property
    def nW(self) -> int:
        return (self.res // self.ws) ** 2

    @property
    def C(self) -> int:
        return self.heads * HD

    @property
    def L(self) -> int:
        return self.res * self.res

    @property
    def nchunk(self) -> int:
        return (self.N + HD - 1) // HD

    def tok(self) -> torch.Tensor:
        """(nW, N) un-shifted token index of (window, slot)."""
        return R.window_token_index(self.res, self.ws, self.shift)

    def slot_regions(self) -> torch.Tensor:
        """(nW, N) region id (0..8) of (window, slot) on the shifted grid."""
        n = self.res // self.ws
        rid = W.shifted_window_region_ids(self.res, self.ws, self.shift)
        return rid.view(n, self.ws, n, self.ws).permute(0, 2, 1, 3).reshape(n * n, self.N)


class Family(NamedTuple):
    q: torch.Tensor          # (B, nW, heads, N, 32) fp32, window order
    k: torch.Tensor          # (B, nW, heads, N, 32)
    table: torch.Tensor      # ((2ws-1)², heads) fp32


def _codes(g: torch.Generator, lead: Tuple[int, int], geo: Geometry, paired: bool) -> torch.Tensor:
    """(*lead, heads, N, 32) of ±1.  paired: slots j and N-1-j share a code."""
    c = torch.randint(0, 2, (*lead, geo.heads, geo.N, HD), generator=g).float() * 2.0 - 1.0
    if paired:
        j = torch.arange(geo.N)
        c = c[..., torch.minimum(j, geo.N - 1 - j), :]
    return c


def _perm_table(g: torch.Generator, geo: Geometry) -> torch.Tensor:
    nt = (2 * geo.ws - 1) ** 2
    vals = torch.linspace(-3.0, 3.0, nt)
    return torch.stack([vals[torch.randperm(nt, generator=g)] for _ in range(geo.heads)], dim=1).contiguous()


@functools.lru_cache(maxsize=None)
def family(name: str, geo: Geometry, per_window: bool = True, seed: int = 0) -> Family:
    """The inputs of one family.  per_window=False: q and k depend on (head, slot) only (what a probe through a qkv product
    with one-hot rows can express); the `mask` family is per window by construction."""
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(name) + seed + 17 * geo.ws + geo.shift)
    lead = (geo.B, geo.nW) if per_window else (1, 1)
    full = (geo.B, geo.nW, geo.heads, geo.N, HD)
    nt = (2 * geo.ws - 1) ** 2
    zero_table = torch.zeros(nt, geo.heads)
    if name == "bias":
        k = torch.randint(-16, 17, (*lead, geo.heads, geo.N, HD), generator=g).float() * 0.25
        return Family(torch.zeros(full), k.expand(full).contiguous(), _perm_table(g, geo))
    if name in ("score", "peaked"):
        code = _codes(g, lead, geo, paired=(name == "peaked")).expand(full).contiguous()
        if name == "score":
            return Family(2.0 * code, code, zero_table)
        return Family(8.0 * code, code, _perm_table(g, geo))
    if name == "mask":
        if not per_window:
            raise ValueError("the mask family's keys follow the window's regions")
        h = torch.tensor(MASK_H)[geo.slot_regions()]                    # (nW, N)
        k = torch.zeros(full)
        k[..., 0] = h[None, :, None, :]
        q = torch.zeros(full)
        q[..., 0] = 8.0
        return Family(q, k, zero_table)
    raise ValueError(name)


def attn_mask(geo: Geometry) -> torch.Tensor:
    """(nW, N, N) fp64 in {0, -100}; all zero without a shift."""
    return W.shifted_window_attn_mask(geo.res, geo.ws, geo.shift).double()


def scores(geo: Geometry, fam: Family, *, rel_index: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
           dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """(B, nW, heads, N, N) pre-softmax scores in `dtype`.  rel_index / mask replace the true ones (reference mutants)."""
    idx = W.relative_position_index(geo.ws) if rel_index is None else rel_index
    m = attn_mask(geo) if mask is None else mask
    bias = fam.table.to(dtype)[idx.reshape(-1)].reshape(geo.N, geo.N, geo.heads).permute(2, 0, 1)
    s = torch.matmul(fam.q.to(dtype) * SCALE, fam.k.to(dtype).transpose(-1, -2)) + bias[None, None]
    return s + m.to(dtype)[None, :, None]


def p_reference(geo: Geometry, fam: Family, **kw) -> torch.Tensor:
    """(B, nW, heads, N, N) probabilities; fp64 unless dtype= says otherwise."""
    return torch.softmax(scores(geo, fam, **kw), dim=-1)


@functools.lru_cache(maxsize=None)
def p_want(name: str, geo: Geometry, per_window: bool = True) -> torch.Tensor:
    """The fp64 reference of a family, computed once and shared (do not write to it)."""
    return p_reference(geo, family(name, geo, per_window))


def masked_pairs(geo: Geometry) -> torch.Tensor:
    """(1, nW, 1, N, N) bool: the pair lies across a region boundary."""
    return (attn_mask(geo) != 0)[None, :, None]


# ------------------------------------------------------------------------------------------------- launches
def one_hot_v(geo: Geometry, r: int) -> torch.Tensor:
    """(heads, N, 32): head h carries key chunk (h + r) % nchunk."""
    v = torch.zeros(geo.heads, geo.N, HD)
    j = torch.arange(geo.N)
    for h in range(geo.heads):
        sel = (j // HD) == (h + r) % geo.nchunk
        v[h, j[sel], j[sel] % HD] = 1.0
    return v


def to_tokens(geo: Geometry, x: torch.Tensor) -> torch.Tensor:
    """(B, nW, heads, N, 32) in window order → (B, L, heads·32) token-major."""
    out = torch.empty(geo.B, geo.L, geo.C, dtype=x.dtype)
    out[:, geo.tok().reshape(-1)] = x.permute(0, 1, 3, 2, 4).reshape(geo.B, geo.nW * geo.N, geo.C)
    return out


def from_tokens(geo: Geometry, x: torch.Tensor) -> torch.Tensor:
    """Inverse of to_tokens: (B·L, heads·32) → (B, nW, heads, N, 32)."""
    x = x.reshape(geo.B, geo.L, geo.C)[:, geo.tok().reshape(-1)]
    return x.reshape(geo.B, geo.nW, geo.N, geo.heads, HD).permute(0, 1, 3, 2, 4)


def qkv_rows(geo: Geometry, fam: Family, r: int) -> torch.Tensor:
    """fp32 [B·L, 3C] qkv buffer (columns (3, heads, 32)) of launch r."""
    v = one_hot_v(geo, r)[None, None].expand(geo.B, geo.nW, -1, -1, -1)
    parts = [to_tokens(geo, t) for t in (fam.q, fam.k, v)]
    return torch.cat(parts, dim=-1).reshape(geo.B * geo.L, 3 * geo.C)


def collect(geo: Geometry, outs) -> torch.Tensor:
    """The nchunk launch outputs [B·L, C] → P (B, nW, heads, N, N) fp64.  Every key column of every head is filled exactly
    once (heads >= nchunk)."""
    assert geo.heads >= geo.nchunk and len(outs) == geo.nchunk
    P = torch.full((geo.B, geo.nW, geo.heads, geo.N, geo.N), float("nan"), dtype=torch.float64)
    for r, o in enumerate(outs):
        o = from_tokens(geo, o.detach().cpu().double())
        for h in range(geo.heads):
            c = (h + r) % geo.nchunk
            n = min(HD, geo.N - HD * c)
            P[:, :, h, :, HD * c:HD * c + n] = o[:, :, h, :, :n]
            if n < HD:      # columns past the last key meet an all-zero V
                assert float(o[:, :, h, :, n:].abs().max()) == 0.0, "output columns past the window's last key are not zero"
    return P


def probe(geo: Geometry, fam: Family, attend: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    """attend: fp32 CPU qkv [B·L, 3C] → the attention output [B·L, C] (any float dtype / device).  Returns P."""
    return collect(geo, [attend(qkv_rows(geo, fam, r)) for r in range(geo.nchunk)])


def oracle_attend(geo: Geometry, fam: Family) -> Callable[[torch.Tensor], torch.Tensor]:
    """The oracle's window_attention_core in fp64 behind the token-major interface of the kernels."""
    idx = W.relative_position_index(geo.ws)
    bias = fam.table.double()[idx.reshape(-1)].reshape(geo.N, geo.N, geo.heads).permute(2, 0, 1)

    def attend(qkv: torch.Tensor) -> torch.Tensor:
        q, k, v = (from_tokens(geo, qkv[:, i * geo.C:(i + 1) * geo.C].double()) for i in range(3))
        o = R.window_attention_core(q, k, v, bias, attn_mask(geo) if geo.shift > 0 else None, SCALE)
        return to_tokens(geo, o.contiguous()).reshape(geo.B * geo.L, geo.C)
    return attend


def attention_fp64(geo: Geometry, qkv: torch.Tensor, table: torch.Tensor, scale: float) -> torch.Tensor:
    """fp64 window attention of an arbitrary token-major qkv [B·L, 3C] → [B·L, C] (the fused kernels' reference)."""
    idx = W.relative_position_index(geo.ws)
    bias = table.double()[idx.reshape(-1)].reshape(geo.N, geo.N, geo.heads).permute(2, 0, 1)
    q, k, v = (from_tokens(geo, qkv[:, i * geo.C:(i + 1) * geo.C].double()) for i in range(3))
    o = R.window_attention_core(q, k, v, bias, attn_mask(geo) if geo.shift > 0 else None, scale)
    return to_tokens(geo, o.contiguous()).reshape(geo.B * geo.L, geo.C)


# ------------------------------------------------------------------------------------------------- comparison
class Verdict(NamedTuple):
    bad: int                 # pairs beyond the bound
    used: float              # max |d| / (rtol·want + atol)
    rel: float               # max |d| / want over the pairs whose bound is relative (rtol·want >= 100·atol)
    where: Tuple[int, ...]   # (b, window, head, query, key) of the pair that uses most of its bound
    got: float
    want: float


def compare(P_got: torch.Tensor, P_want: torch.Tensor, rtol: float, atol: float) -> Verdict:
    assert P_got.shape == P_want.shape, (P_got.shape, P_want.shape)
    d = (P_got - P_want).abs()
    d = torch.where(torch.isfinite(d), d, torch.full_like(d, float("inf")))       # a NaN / inf output is beyond any bound
    bound = rtol * P_want + atol
    ratio = d / bound
    at = int(ratio.argmax())
    where = tuple(int(i) for i in torch.unravel_index(torch.tensor(at), ratio.shape))
    relmask = rtol * P_want >= 100.0 * atol
    rel = float((d[relmask] / P_want[relmask]).max()) if bool(relmask.any()) else 0.0
    return Verdict(int((d > bound).sum()), float(ratio.reshape(-1)[at]), rel, where,
                   float(P_got.reshape(-1)[at]), float(P_want.reshape(-1)[at]))


def assert_pairs(P_got: torch.Tensor, P_want: torch.Tensor, fmt: str, what: str) -> Verdict:
    rtol, atol = BOUNDS[fmt]
    v = compare(P_got, P_want, rtol, atol)
    print(f"PROBE {what}: used {v.used:.3e} of the bound, worst rel {v.rel:.3e}, at (b, win, head, query, key) = {v.where}")
    assert v.bad == 0, (f"{what}: {v.bad} of {P_want.numel()} pairs beyond |d| <= {rtol}·P + {atol:.1e}; worst at "
                        f"(b, window, head, query, key) = {v.where}: got {v.got:.6e}, want {v.want:.6e}")
    return v


def assert_mask_is_additive(P_got: torch.Tensor, P_want: torch.Tensor, geo: Geometry, fmt: str, what: str) -> int:
    """Masked pairs whose probability the output format can tell from zero must not be zero: the mask is -100, not -inf.
    The floor follows from the bound: rtol·P + atol < P  ⇔  P > atol / (1 − rtol).  Returns how many pairs were above it."""
    rtol, atol = BOUNDS[fmt]
    floor = atol / (1.0 - rtol)
    sel = masked_pairs(geo).expand_as(P_want) & (P_want > floor)
    n = int(sel.sum())
    if n:
        assert bool((P_got[sel] > 0).all()), f"{what}: {int((P_got[sel] <= 0).sum())} of {n} masked pairs above {floor:.1e} came back 0"
    return n
