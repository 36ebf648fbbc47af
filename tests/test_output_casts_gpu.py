"""Every store path that narrows an fp32 result to bf16, fp16, e4m3 or split fp16 ("h2"), at the edges of the format: rounding
ties above even and odd significands, the subnormal range, the largest finite value, values past it, ±inf and NaN
(output_cast_refs.PATTERNS; test_output_casts_host.py shows that the references are right and that a truncating, a
round-half-up, a non-saturating or a NaN-hiding cast differs from them on these patterns).

The launches are arranged so that the arithmetic in front of the cast is exact and the output is cast(an input) bit for bit:
  * GEMM epilogues: A is all zero bytes, so alpha·col_scale·(A·Wᵀ) is exactly 0 and out = cast(bias) (bias per column, two
    rotations of the pattern list over the columns, and per row once per family), or out = cast(0 + residual[m][n]) where the
    family adds the fp32 residual in front of the cast (bf16, f32, x3: every element its own value).  Shapes and leading
    dimensions are those of containment_cases.cases, which reach the whole-line, the 16-byte vector, the scalar tail and the
    ragged-last-row-tile stores of every selectable tile; the A-resident tiles get one whole tile.
  * LayerNorm and patch-merge LayerNorm: gamma = 0, so out = cast(beta).
  * odic_cast_f32_to_h2 on ±inf and NaN (test_frontend_shapes_gpu.py has the finite values).

Comparison is bitwise (OC.mismatch): two zeros of different sign count as equal, and every NaN must come out a NaN.

Out of scope, because their outputs cannot reach an edge: window attention writes convex combinations of its (finite) V rows,
and stcexp_normalize writes values in [0, 1]·scale.  The fused Swin kernels (qkv + attention, MLP) are bit-identical to
launches covered here, which test_swin_mlp_gpu.py / test_swin_qkv_attention_tiled_gpu.py / test_hip_ops.py pin.  The ReLU launches leave the NaN patterns out:
what an ACTIVATION makes of a NaN is not the cast's rule (ODIC_ACT_RELU is a plain max, which returns 0 for a NaN).
"""
import pytest
import torch

import frontend_refs as FR
import output_cast_refs as OC
from containment_cases import APANEL, BM, KDEF, cases as _cases, panel_candidates, tiled_tiles
from guards import H2, guarded

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn
FMT = {BF16: "bf16", F16: "fp16", FP8: "e4m3", H2: "h2"}
#: the narrow outputs of each family (an fp32 output has no cast)
NARROW = {"bf16": (BF16,), "f32": (BF16,), "fp8": (F16, FP8), "fp16": (F16, FP8), "x3": (H2,)}
RESIDUAL_BEFORE_CAST = ("bf16", "f32", "x3")      # out = act(...) + residual, THEN the cast (csrc/gemm_*.hip)
ROTATIONS = (0, 13)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from on_device_image_captioning_amd import _hip, ops as o
    _hip.load()
    return o


_W = {}


def _operands(ops, fam, M, N, K):
    """(A = zero bytes, W = random finite values) of the family's input type; W is made once per (family, N, K)."""
    key = (fam, N, K)
    if key not in _W:
        w = torch.randn(N, K, generator=torch.Generator().manual_seed(N + K))
        _W[key] = {"bf16": lambda: w.bfloat16(), "f32": lambda: w, "fp16": lambda: w.half(), "fp8": lambda: w.to(FP8),
                   "x3": lambda: ops.h2_from_f32(w)}[fam]().to(DEV)
    W = _W[key]
    return torch.zeros(M, K, dtype=W.dtype, device=DEV), W


def _col_scale(fam, N):
    if fam not in ("fp8", "fp16"):
        return None
    return (0.5 + torch.rand(N, generator=torch.Generator().manual_seed(N))).to(DEV)       # != 1; 0 · cs is still 0


def _launch(ops, fam, tile, odt, M, N, ldc, K, *, bias=None, bias_axis=0, residual=None, act=0):
    """One product with A = 0 into a poisoned [M, ldc] buffer; returns the codes [M, N] of what it wrote."""
    A, W = _operands(ops, fam, M, N, K)
    o = guarded(M, N, ldc, odt, DEV)
    ldr = None if residual is None else residual.shape[1]
    ops.gemm(A, W, None if bias is None else bias.to(DEV), None if residual is None else residual.to(DEV), out=o.t, act=act,
             alpha=1.0, bias_axis=bias_axis, M=M, N=N, K=K, lda=K, ldw=K, ldr=ldr, ldc=ldc, tile_cfg=tile,
             col_scale=_col_scale(fam, N), out_scale=1.0)
    torch.cuda.synchronize()
    t = o.t.cpu()
    if odt == H2:
        return OC.codes_of("h2", t)[:, :N]
    return OC.codes_of(FMT[odt], t[:, :N])


def _check(fmt, got, x, what):
    """got [M, N] codes against the reference cast of the fp32 values x [M, N]."""
    want = OC.ref_codes(fmt, x)
    bad = OC.mismatch(fmt, got, want)
    if bool(bad.any()):
        rows = [(m, n, hex(int(x.view(torch.int32)[m, n]) & 0xFFFFFFFF), [hex(int(v)) for v in got[m, n].reshape(-1)],
                 [hex(int(v)) for v in want[m, n].reshape(-1)]) for m, n in bad.nonzero()[:12].tolist()]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the reference cast; "
                             f"(row, column, fp32 bits, got, want): {rows}")
    nan = torch.isnan(x)
    assert bool(OC.is_nan_code(fmt, got)[nan].all()), f"{what}: a NaN did not stay a NaN"


def _shapes(fam, tile, odt):
    """The distinct (M, N, ldc) of the containment plan for this tile and output type."""
    return list(dict.fromkeys((c.M, c.N, c.ldc) for c in _cases(fam, BM[fam][tile], odt)))


def _bias_case(ops, fam, tile, odt, M, N, ldc, K, r, axis=0, act=0):
    fmt = FMT[odt]
    n = N if axis == 0 else M
    bias = OC.rotated(fmt, n, r, nan=act == 0)
    got = _launch(ops, fam, tile, odt, M, N, ldc, K, bias=bias, bias_axis=axis, act=act)
    x = (bias[None, :] if axis == 0 else bias[:, None]).expand(M, N).contiguous()
    if act == 2:
        assert bool((x < 0).any()) and bool((x > 0).any())
        x = torch.relu(x)
    _check(fmt, got, x, f"{fam} tile {tile} -> {fmt} {M}x{N} ldc {ldc} bias axis {axis} rotation {r} act {act}")


@pytest.mark.parametrize("fam", ["bf16", "f32", "fp8", "fp16", "x3"])
def test_gemm_epilogue_casts_bias_every_tile_and_store_path(ops, fam):
    for odt in NARROW[fam]:
        for tile in tiled_tiles(ops, fam):
            for M, N, ldc in _shapes(fam, tile, odt):
                for r in ROTATIONS:
                    _bias_case(ops, fam, tile, odt, M, N, ldc, KDEF[fam], r)


@pytest.mark.parametrize("fam", ["bf16", "f32", "fp8", "fp16", "x3"])
def test_gemm_epilogue_casts_row_bias_and_relu(ops, fam):
    for odt in NARROW[fam]:
        M, N, ldc = _shapes(fam, -1, odt)[0]
        _bias_case(ops, fam, -1, odt, M, N, ldc, KDEF[fam], 0, axis=1)
        _bias_case(ops, fam, -1, odt, M, N, ldc, KDEF[fam], 0, act=2)       # ReLU: negatives -> +0, positives unchanged


@pytest.mark.parametrize("fam", RESIDUAL_BEFORE_CAST)
def test_gemm_epilogue_casts_residual_every_tile(ops, fam):
    """out = cast(0 + residual[m][n]), residual[m][n] = patterns[(7m + n) % P]: every element its own value.  ldr = N rounded
    up to 4 (zero padding), so that the 16-byte residual loads run wherever the output's leading dimension allows them."""
    for odt in NARROW[fam]:
        fmt = FMT[odt]
        for tile in tiled_tiles(ops, fam):
            for M, N, ldc in _shapes(fam, tile, odt):
                ldr = -(-N // 4) * 4
                res = torch.zeros(M, ldr)
                vals = OC.take(fmt, 7 * torch.arange(M)[:, None] + torch.arange(N)[None, :])
                res.view(torch.int32)[:, :N] = vals.view(torch.int32)
                got = _launch(ops, fam, tile, odt, M, N, ldc, KDEF[fam], residual=res)
                _check(fmt, got, res[:, :N].contiguous(), f"{fam} tile {tile} -> {fmt} {M}x{N} ldc {ldc} residual")


@pytest.mark.parametrize("fam", ["bf16", "x3"])
def test_gemm_a_resident_epilogue_casts(ops, fam):
    """The A-resident tiles take whole tiles only: one tile, K as the tile fixes it, both rotations."""
    odt = NARROW[fam][0]
    tiles = panel_candidates(ops, fam)
    assert tiles
    for tile in tiles:
        bm, bnc, K = APANEL[fam][tile]
        for r in ROTATIONS:
            _bias_case(ops, fam, tile, odt, bm, bnc, bnc, K, r)


# ============================================================================================== LayerNorm
def _vpl(C):
    return next(v for v in (1, 2, 4, 8, 16, 32) if C // 4 <= 64 * v)


def _ln_widths(fmt):
    """The first and the last width of each VPL instantiation among FR.LAYERNORM_CASES that the format takes (h2: C % 8)."""
    by = {}
    for c in FR.LAYERNORM_CASES:
        if fmt != "h2" or c.C % 8 == 0:
            by.setdefault(_vpl(c.C), set()).add(c.C)
    assert sorted(by) == [1, 2, 4, 8, 16, 32]
    return sorted({w for s in by.values() for w in (min(s), max(s))})


def _ln_out(ops, odt):
    return ops.H2_DTYPE if odt == H2 else odt


@pytest.mark.parametrize("odt", [BF16, FP8, H2], ids=["bf16", "e4m3", "h2"])
def test_layernorm_casts_beta(ops, odt):
    fmt, M = FMT[odt], 5
    for C in _ln_widths(fmt):
        x = torch.randn(M, C, generator=torch.Generator().manual_seed(C)) * 3.0
        for r in ROTATIONS:
            beta = OC.rotated(fmt, C, r)
            got = ops.layernorm(x.to(DEV), torch.zeros(C, device=DEV), beta.to(DEV), out_dtype=_ln_out(ops, odt)).cpu()
            assert got.shape == (M, C)
            _check(fmt, OC.codes_of(fmt, got), beta[None, :].expand(M, C).contiguous(), f"layernorm -> {fmt} C {C} rotation {r}")


@pytest.mark.parametrize("odt", [BF16, H2], ids=["bf16", "h2"])
@pytest.mark.parametrize("case", [FR.PatchMergeCase(2, 10, 36, ()), FR.PatchMergeCase(1, 4, 2048, ())], ids=lambda c: c.name)
def test_patch_merge_layernorm_casts_beta(ops, case, odt):
    fmt, C4 = FMT[odt], 4 * case.C
    x, _, _ = FR.patch_merge_inputs(case)
    rows = case.B * (case.res // 2) ** 2
    for r in ROTATIONS:
        beta = OC.rotated(fmt, C4, r)
        got = ops.patch_merge_layernorm(x.to(DEV), torch.zeros(C4, device=DEV), beta.to(DEV), case.B, case.res, case.C,
                                        out_dtype=_ln_out(ops, odt)).cpu().reshape(rows, C4)
        _check(fmt, OC.codes_of(fmt, got), beta[None, :].expand(rows, C4).contiguous(), f"patch merge {case.name} -> {fmt} rotation {r}")


# ============================================================================================== the stand-alone h2 cast
def test_cast_h2_inf_and_nan(ops):
    """±inf saturate to ±65504 (lo = 0); a NaN leaves as a NaN (test_cast_h2_finite_special_values_bytewise: finite values)."""
    x = OC.values(OC.PATTERNS["h2"] + [0] * (-len(OC.PATTERNS["h2"]) % 8)).reshape(1, -1)
    x = torch.cat([x, OC.values((FR.CAST_INF_BITS + FR.CAST_NAN_BITS) * (x.shape[1] // 8)).reshape(1, -1)])
    got = ops.cast_h2(x.to(DEV)).cpu()
    _check("h2", OC.codes_of("h2", got), x, "odic_cast_f32_to_h2")
    assert bool(torch.isinf(x).any()) and bool(torch.isnan(x).any())
