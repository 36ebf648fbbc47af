"""References, inputs and case lists for the kernels at the front of the pipeline (csrc/norm.hip: patch embed, LayerNorm,
patch-merge LayerNorm) and the encoder's glue (csrc/encoder_ops.hip: stcexp_normalize, selector_mix), shared by
test_frontend_shapes_host.py (no GPU: the references agree with the oracle, every bound is met by a float32 evaluation of the
same formula) and test_frontend_shapes_gpu.py (the HIP kernels against the references).

The references are plain torch restatements of the operations, float64 by default; `dtype=torch.float32` evaluates the same
formula in float32 (the host test's stand-in for "an fp32 implementation with another summation order").  Nothing here knows
about `Geometry`, and nothing here is derived from a kernel's output.

Not a conftest: import it (`import frontend_refs as FR`), like the *_model.py modules.
"""
from __future__ import annotations

from typing import NamedTuple, Sequence, Tuple

import torch
import torch.nn.functional as F

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16

#: the project's bounds for these kernels (tests/test_hip_ops.py): fp32 outputs within 2e-5 of the reference's largest
#: magnitude (summation order only), bf16 outputs within 5e-3 (test_layernorm: order + the final rounding, 2^-9 = 2.0e-3)
BOUND_F32 = 2e-5
BOUND_BF16 = 5e-3


def bound_of(odt) -> float:
    return BOUND_F32 if odt == F32 else BOUND_BF16


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def max_err(got: torch.Tensor, want: torch.Tensor) -> Tuple[float, float]:
    """(largest absolute error, the reference's largest magnitude), both in float64 on the CPU."""
    got, want = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max()), float(want.abs().max())


def assert_within(got, want, bound, what, scale=None):
    """|got - want| <= bound * scale everywhere; scale = the reference's largest magnitude unless given.  A scale of 0 (a
    table that must be all zeros) asks for exact zeros.  The figure is printed before it is asserted."""
    err, ref_scale = max_err(got, want)
    scale = ref_scale if scale is None else scale
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, ratio {err / scale if scale else 0.0:.3e} (bound {bound:g})")
    assert bool(torch.isfinite(got.detach().cpu().to(F64)).all()), f"{what}: non-finite values"
    assert err <= bound * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (bound {bound:g})"


# =====================================================================================================================
# patch embed
# =====================================================================================================================
def patch_embed_ref(img, w, b, gamma, beta, patch, eps=1e-5, dtype=F64):
    """Conv2d(k = s = patch) -> (B, L, C) -> LayerNorm(C).  img [B, in_chans, H, W]; w [C, in_chans·patch²] as the entry
    point takes it."""
    C, cin = w.shape[0], img.shape[1]
    y = F.conv2d(img.to(dtype), w.to(dtype).reshape(C, cin, patch, patch), b.to(dtype), stride=patch)
    return F.layer_norm(y.flatten(2).transpose(1, 2), (C,), gamma.to(dtype), beta.to(dtype), eps)


class PatchEmbedCase(NamedTuple):
    B: int
    in_chans: int
    H: int
    W: int
    C: int
    misaligned_w: bool = False      # w = a contiguous view one float into a larger buffer: the scalar transpose path

    @property
    def name(self):
        return f"B{self.B}_c{self.in_chans}_{self.H}x{self.W}_C{self.C}" + ("_w_off_by_one_float" if self.misaligned_w else "")


#: a block of the kernel owns 64 consecutive tokens of the flat (image, token) list
PATCH_EMBED_CASES = [
    PatchEmbedCase(5, 3, 16, 16, 64),          # 16 tokens per image: one block covers four images
    PatchEmbedCase(3, 3, 40, 24, 96),          # 60 tokens per image, H != W: blocks 0 and 1 end with the head of the next image
    PatchEmbedCase(4, 3, 20, 24, 96),          # 30 tokens per image, H != W: block 0 = images 0, 1 and the head of image 2
    PatchEmbedCase(2, 3, 36, 40, 128),         # 90 tokens per image: blocks span two images, the last one has 52 tokens
    PatchEmbedCase(1, 1, 32, 32, 192),         # K = 16, exactly one full block
    PatchEmbedCase(3, 4, 24, 48, 256),         # K = 64 (the limit) and the largest LDS request
    PatchEmbedCase(1, 3, 4, 4, 96),            # a single token
    PatchEmbedCase(2, 3, 36, 40, 128, True),   # case 3 with w not 16-byte aligned
]

#: (B, in_chans, H, W, patch, C) the entry point must refuse, writing nothing
PATCH_EMBED_REFUSED = [
    (2, 5, 16, 16, 4, 96),     # K = 80 > 64
    (2, 3, 16, 16, 4, 80),     # C = 80: no instantiation
    (2, 3, 16, 16, 4, 100),    # C % 16 != 0
    (2, 3, 18, 16, 4, 96),     # H % patch != 0
    (2, 3, 16, 16, 2, 96),     # patch = 2
]


def patch_embed_inputs(c: PatchEmbedCase, patch=4):
    """img, w [C, K], b, gamma, beta (float32, CPU).  Every image has its own seed and its own constant offset: a token read
    from another image (or from another row of its own) does not reproduce the right one."""
    K = c.in_chans * patch * patch
    img = torch.stack([_randn(c.in_chans, c.H, c.W, seed=100 + 7 * i) + (0.75 * i - 1.5) for i in range(c.B)])
    w = _randn(c.C, K, seed=11) * 0.2
    b = _randn(c.C, seed=12) * 0.1
    return img, w, b, 1 + 0.1 * _randn(c.C, seed=13), 0.1 * _randn(c.C, seed=14)


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
def layernorm_ref(x, gamma, beta, eps=1e-5, dtype=F64):
    return F.layer_norm(x.to(dtype), (x.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)


class LayerNormCase(NamedTuple):
    M: int
    C: int
    pad: int            # ldx = C + pad
    odts: tuple
    off_err: float      # float32 CPU layer_norm against float64 on the row of randn + 30, relative to the case's scale, as
                        # test_layernorm_offset_row_error_is_recorded measured it (0: the case has no such row)

    @property
    def ldx(self):
        return self.C + self.pad

    @property
    def name(self):
        return f"M{self.M}_C{self.C}" + (f"_ldx{self.ldx}" if self.pad else "")


_BOTH = (F32, BF16)
#: launch_ln picks VPL (float4 per lane) in {1, 2, 4, 8, 16, 32} by C/4 <= 64·VPL: each pair below is the last width of one
#: instantiation and the first of the next; 4 and 8 are the narrowest rows, 8188 / 8192 the widest the entry point takes.
#: The last field of each case is off_err as measured (x86-64, torch's vectorised CPU layer_norm): 9e-8 to 7e-7, so four times
#: it stays under 2e-5 and the offset row's bound is the project's 2e-5 in every case.
LAYERNORM_CASES = [
    LayerNormCase(5, 4, 0, (F32,), 4.281e-07),
    LayerNormCase(5, 8, 0, (F32,), 5.283e-07),
    LayerNormCase(5, 256, 0, _BOTH, 4.977e-07),
    LayerNormCase(5, 260, 0, _BOTH, 4.144e-07),
    LayerNormCase(5, 512, 0, _BOTH, 2.041e-07),
    LayerNormCase(5, 516, 0, _BOTH, 6.632e-07),
    LayerNormCase(5, 1024, 0, _BOTH, 4.196e-07),
    LayerNormCase(5, 1028, 0, _BOTH, 3.481e-07),
    LayerNormCase(5, 2048, 0, _BOTH, 2.595e-07),
    LayerNormCase(5, 2052, 0, _BOTH, 2.096e-07),
    LayerNormCase(5, 4096, 0, _BOTH, 3.904e-07),
    LayerNormCase(5, 4100, 0, _BOTH, 9.082e-08),
    LayerNormCase(5, 8188, 0, (F32,), 1.882e-07),
    LayerNormCase(5, 8192, 0, (F32,), 1.171e-07),
    LayerNormCase(1, 96, 0, (F32,), 0.0),           # one row: a block with three idle waves
    LayerNormCase(1, 260, 0, (F32,), 0.0),
    LayerNormCase(1027, 96, 0, (F32,), 5.381e-07),  # M >= 1024 (raised wave priority), last block 3 rows
    LayerNormCase(1027, 260, 0, (F32,), 3.031e-07),
    LayerNormCase(5, 260, 8, (F32,), 4.144e-07),    # ldx = C + 8
    LayerNormCase(5, 4100, 8, (F32,), 9.082e-08),
]
LAYERNORM_REFUSED_C = [8196, 6]
LN_CONST = 3.0


def layernorm_rows(M):
    """Row indices (constant, zero, offset) of a case with M rows, or None for each when M < 4: the last three rows, so that
    with M = 1027 they sit in the partial last block."""
    return (M - 3, M - 2, M - 1) if M >= 4 else (None, None, None)


def layernorm_inputs(c: LayerNormCase):
    """x [M, C] (float32, CPU; the caller lays it out with ldx), gamma, beta.  Random rows at scale 3; one row of the constant
    LN_CONST, one of zeros (both normalise to beta exactly in exact arithmetic) and one of randn + 30 (a mean 30 times the
    spread: a one-pass E[x²] - E[x]² variance loses 3 digits there)."""
    x = _randn(c.M, c.C, seed=1000 + c.C) * 3.0
    rc, rz, ro = layernorm_rows(c.M)
    if rc is not None:
        x[rc] = LN_CONST
        x[rz] = 0.0
        x[ro] = _randn(c.C, seed=2000 + c.C) + 30.0
    return x, 1 + 0.1 * _randn(c.C, seed=2), 0.1 * _randn(c.C, seed=3)


def layernorm_offset_bound(c: LayerNormCase) -> float:
    """The fp32 bound of the randn + 30 row: the larger of the project's 2e-5 and four times what float32 CPU layer_norm
    itself loses on that row (the factor covers another summation order, not a one-pass variance)."""
    return max(BOUND_F32, 4.0 * c.off_err)


# =====================================================================================================================
# patch merging + LayerNorm
# =====================================================================================================================
def patch_merge_ln_ref(x, gamma, beta, B, res, C, eps=1e-5, dtype=F64):
    """x [B, res², C] -> [B, (res/2)², 4C]: the 2x2 neighbourhood in the order (0,0), (1,0), (0,1), (1,1) (row offset, column
    offset), concatenated along the channels, then LayerNorm(4C)."""
    g = x.to(dtype).reshape(B, res // 2, 2, res // 2, 2, C)
    cat = torch.cat([g[:, :, 0, :, 0], g[:, :, 1, :, 0], g[:, :, 0, :, 1], g[:, :, 1, :, 1]], -1)
    cat = cat.reshape(B, (res // 2) ** 2, 4 * C)
    return F.layer_norm(cat, (4 * C,), gamma.to(dtype), beta.to(dtype), eps)


class PatchMergeCase(NamedTuple):
    B: int
    res: int
    C: int
    odts: tuple

    @property
    def name(self):
        return f"B{self.B}_res{self.res}_C{self.C}"


PATCH_MERGE_CASES = [
    PatchMergeCase(1, 2, 4, (F32,)),           # one output row of 16 channels: every float4 is a whole segment
    PatchMergeCase(3, 6, 8, (F32,)),
    PatchMergeCase(2, 10, 36, _BOTH),          # C/4 = 9: lanes 9, 18, 27 start a segment, a wave's 64 float4s straddle them
    PatchMergeCase(2, 14, 192, (F32,)),        # 4C/4 = 192: three float4 per lane (VPL 4), 98 rows
    PatchMergeCase(1, 4, 2048, _BOTH),         # 4C = 8192, the limit
]
PATCH_MERGE_REFUSED = [(2, 5, 8), (2, 6, 6), (1, 4, 2052)]      # res odd, C % 4 != 0, 4C > 8192


def patch_merge_inputs(c: PatchMergeCase):
    """x [B, res², C], gamma, beta [4C].  Every token carries its own offset, so a swapped neighbour shows."""
    ntok = c.B * c.res * c.res
    x = _randn(ntok, c.C, seed=50 + c.C) + torch.linspace(-2.0, 2.0, ntok)[:, None]
    return x.reshape(c.B, c.res * c.res, c.C), 1 + 0.1 * _randn(4 * c.C, seed=2), 0.1 * _randn(4 * c.C, seed=3)


# =====================================================================================================================
# stcexp_normalize
# =====================================================================================================================
def stcexp_ref(z, enc_len, groups: Sequence[int], eps=1e-9, dtype=F64):
    """z [B, nq, S] -> (pos_fw, neg_fw [B, nq, S], pos_bw, neg_bw [B, S, nq]).  Forward: relu(±z) masked to the first
    enc_len[b] keys, every row divided by (its sum + eps).  Backward: relu(±zᵀ), NOT masked, every column group divided by
    (its sum + eps), then by len(groups)."""
    zd = z.to(dtype)
    S = zd.shape[-1]
    valid = (torch.arange(S)[None, :] < torch.as_tensor(enc_len)[:, None]).to(dtype)[:, None, :]
    pf, nf = torch.relu(zd) * valid, torch.relu(-zd) * valid
    pf, nf = pf / (pf.sum(-1, keepdim=True) + eps), nf / (nf.sum(-1, keepdim=True) + eps)
    zt = zd.transpose(1, 2)
    pb, nb = torch.relu(zt).clone(), torch.relu(-zt).clone()
    lo = 0
    for n in groups:
        sl = slice(lo, lo + n)
        pb[..., sl] = pb[..., sl] / (pb[..., sl].sum(-1, keepdim=True) + eps)
        nb[..., sl] = nb[..., sl] / (nb[..., sl].sum(-1, keepdim=True) + eps)
        lo += n
    return pf, nf, pb / len(groups), nb / len(groups)


#: stcexp_colsum_kernel gives each of 16 slices every 16th query of a group and loads eight of them per trip while
#: slice + 112 < group size.  The production list: 2 to 32 queries per slice.  The second list: groups narrower than the 16
#: slices (1, 15), exactly one query per slice (16), one slice with two (17), the unrolled loop not entered by any slice
#: (112), entered by slice 0 alone (113), by every slice exactly once (128), once plus a remainder trip for slice 0 (129),
#: and twice by slice 0, once plus the longest remainder (7 trips) by the others (241); nq = 772 = 24·32 + 4 leaves the transpose kernel a ragged last tile.
STCEXP_GROUPS = [(32, 64, 128, 256, 512), (1, 15, 16, 17, 112, 113, 128, 129, 241)]
STCEXP_S = [144, 33]
STCEXP_B = 3
STCEXP_NEG_ROW = 5          # (image 0) a query row that is negative at every key: its positive forward row is exact zeros


def stcexp_widest(groups):
    """(first query, size) of the widest group."""
    g = max(range(len(groups)), key=lambda i: groups[i])
    return sum(groups[:g]), groups[g]


def stcexp_pos_col(S):
    return min(7, S - 1)    # (image 0) a key column positive over the widest group: its negative backward column is zeros


def stcexp_inputs(groups, S):
    """z [3, nq, S] at scale 2 with exact 0.0 and -0.0 sprinkled in, the all-negative row and the all-positive column;
    enc_len = (S, 1, 0)."""
    nq = sum(groups)
    z = _randn(STCEXP_B, nq, S, seed=7 + S) * 2.0
    u = torch.rand(STCEXP_B, nq, S, generator=torch.Generator().manual_seed(8 + S))
    z[u < 0.02] = 0.0
    z[u > 0.98] = -0.0
    q0, n = stcexp_widest(groups)
    assert not q0 <= STCEXP_NEG_ROW < q0 + n
    z[0, STCEXP_NEG_ROW, :] = -(z[0, STCEXP_NEG_ROW, :].abs() + 0.01)
    col = stcexp_pos_col(S)
    z[0, q0:q0 + n, col] = z[0, q0:q0 + n, col].abs() + 0.01
    return z, torch.tensor([S, 1, 0], dtype=torch.int32)


def assert_stcexp_tables(got, want, groups, bound, what):
    """The four tables, each against its reference with the scale taken per image and per query group (rows of the forward
    tables, columns of the backward ones): entries of the 512-wide group are 64 times smaller than the 8-wide group's, and an
    image with one valid key has forward entries of 1.  A (image, group) whose reference is all zeros must be exact zeros."""
    for name, gt, wt, axis in zip(("pos_fw", "neg_fw", "pos_bw", "neg_bw"), got, want, (1, 1, 2, 2)):
        gt, wt = gt.detach().cpu().to(F64), wt.detach().cpu().to(F64)
        assert gt.shape == wt.shape, (name, gt.shape, wt.shape)
        assert bool(torch.isfinite(gt).all()), f"{what} {name}: non-finite values"
        worst = 0.0
        for b in range(wt.shape[0]):
            lo = 0
            for gi, n in enumerate(groups):
                g_, w_ = gt[b].narrow(axis - 1, lo, n), wt[b].narrow(axis - 1, lo, n)
                err, scale = float((g_ - w_).abs().max()), float(w_.abs().max())
                assert err <= bound * scale, (f"{what} {name}: image {b}, group {gi} ({n} queries): max err {err:.3e} vs "
                                              f"scale {scale:.3e} (bound {bound:g})")
                worst = max(worst, err / scale if scale else 0.0)
                lo += n
        print(f"{what} {name}: worst err / group scale {worst:.3e} (bound {bound:g})")


# =====================================================================================================================
# selector mix
# =====================================================================================================================
def selector_mix_ref(x, sel, a, b, dtype=F64):
    sg = torch.sigmoid(sel.to(dtype))
    return x.to(dtype) + sg * a.to(dtype) + (1 - sg) * b.to(dtype)


SELECTOR_M, SELECTOR_D = 3, 20
SELECTOR_LDS = (21, 23, 25, 27, 29)                        # x, selector, a, b, out
SELECTOR_EXTREMES = (100.0, -100.0, 20.0, -20.0, 0.0)      # written into columns 0..4 of every row


def selector_inputs():
    x, sel, a, b = (_randn(SELECTOR_M, SELECTOR_D, seed=30 + i) for i in range(4))
    sel = sel * 2.0
    for j, v in enumerate(SELECTOR_EXTREMES):
        sel[:, j] = v
    return x, sel, a, b


# =====================================================================================================================
# casts
# =====================================================================================================================
def _bits(words):
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32).view(torch.float32)


#: fp32 bit patterns: ±0; subnormals (smallest, a middle one, the largest, both signs); ties of the bf16 rounding (low half
#: 0x8000) above an even and above an odd kept half, both signs, with their neighbours one ulp off the tie; ordinary values; tiny
#: values in and under the fp16 subnormal range (the split-fp16 cast); the largest finite float (bf16: rounds to inf; split
#: fp16: saturates at 65504)
CAST_FINITE_BITS = [
    0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00012345, 0x80012345, 0x007FFFFF, 0x807FFFFF,
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,
    0x3F800000, 0xC0490FDB, 0x42F6E979, 0x358637BD, 0x33000000, 0xB3000000, 0x32FFFFFF, 0x33800000,
    0x477FE000, 0x477FF000, 0xC77FF000, 0x47800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x00800000,
]
CAST_INF_BITS = [0x7F800000, 0xFF800000, 0x3F800000, 0x00000000]
#: NaNs: quiet, one whose payload lives in the low half only (truncation would turn it into inf), negative, all ones
CAST_NAN_BITS = [0x7FC00000, 0x7F800001, 0xFFC00001, 0xFFFFFFFF]


def cast_finite_row():
    return _bits(CAST_FINITE_BITS).reshape(1, -1)


def cast_special_rows():
    """[2, 40]: row 0 = the finite values, ±inf, 1, 0 and four NaNs; row 1 = ordinary values.  Returns (x, NaN mask)."""
    r0 = _bits(CAST_FINITE_BITS + CAST_INF_BITS + CAST_NAN_BITS)
    x = torch.stack([r0, _randn(r0.numel(), seed=77)])
    return x, torch.isnan(x)
