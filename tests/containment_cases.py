"""The GEMM case plan of the containment tests, as plain data: which (family, tile configuration, output type, shape, layout,
epilogue) cases tests/test_containment_gpu.py launches.  Kept apart from the launches so that the plan itself is checked
WITHOUT a GPU (tests/test_guards.py): every selectable tile gets a ragged-M, a ragged-N and an ldc > N case, and every shape
satisfies the dispatch code's constraints.  The GPU tests walk the same generators and let any refusal by the library fail, so
a case in the plan is a case that ran.

Tile heights come from the tile tables of csrc/gemm_*.hip themselves (parsed below), not from a copy.
"""
import os
import re

import torch

from guards import H2

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FP8 = torch.float8_e4m3fn
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "on_device_image_captioning_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def tile_heights(name):
    """{tile_cfg: rows of one block's tile} from the `case c: return launch...<NWM, NWN, MI, ...>` lines (BM = NWM·MI·16)."""
    out = {}
    for c1, c2, nwm, mi in re.findall(r"case (\d+):(?: case (\d+):)? return launch(?:_cfg|_persist)?<(\d+), \d+, (\d+),", _src(name)):
        for c in (c1, c2):
            if c:
                out.setdefault(int(c), int(nwm) * int(mi) * 16)
    return out


def panel_tiles(name):
    """{tile_cfg: (BM, BNC, K)} of the A-resident kernels: `case c: return launch_apanel<MI, NI, KT ...>` (bf16: K = 64·KT) /
    `tile_cfg == c) return launch_panel<MI, NI, KT>` (split fp16: K = 32·KT); BM = 4·MI·16, BNC = NI·16."""
    src, out = _src(name), {}
    for c, mi, ni, kt in re.findall(r"case (\d+): return launch_apanel<(\d+), (\d+), (\d+)", src):
        out[int(c)] = (4 * int(mi) * 16, int(ni) * 16, 64 * int(kt))
    for c, mi, ni, kt in re.findall(r"tile_cfg == (\d+)\) return launch_panel<(\d+), (\d+), (\d+)>", src):
        out[int(c)] = (4 * int(mi) * 16, int(ni) * 16, 32 * int(kt))
    return out


_LOWP = tile_heights("gemm_lowp.hip")
_F32_BM = int(re.search(r"constexpr int BM = (\d+)", _src("gemm_f32.hip")).group(1))
# -1 (the built-in choice) starts from the 128-row tile in the three MFMA families; fp8 5..9 are 0..4 on the block-scaled MFMA
BM = {"bf16": {-1: 128, **tile_heights("gemm_bf16.hip")},
      "x3": {-1: 128, **tile_heights("gemm_x3.hip")},
      "fp8": {-1: 128, **{c: _LOWP[c % 5] for c in range(10)}},
      "fp16": {-1: 128, **{c: _LOWP[c] for c in range(3)}},
      "f32": {c: _F32_BM for c in (-1, 0, 1, 2, 3)}}               # (3: the 64 x 64 tile kernel instead of the skinny-M one)
APANEL = {"bf16": panel_tiles("gemm_bf16.hip"), "x3": panel_tiles("gemm_x3.hip")}
ODTS = {"bf16": (F32, BF16), "x3": (F32, H2), "fp8": (F32, F16, FP8), "fp16": (F32, F16, FP8), "f32": (F32, BF16)}
KDEF = {"bf16": 192, "x3": 96, "fp8": 128, "fp16": 64, "f32": 48}      # fp8 128: the block-scaled tiles 5-9 need K % 128 == 0
KMULT = {"bf16": 64, "x3": 32, "fp8": 64, "fp16": 32, "f32": 1}        # the dispatch code's K granularity
KPAD = {"bf16": 8, "x3": 8, "fp8": 16, "fp16": 8, "f32": 4}            # smallest legal step of lda / ldw above K
BATCHED = ("bf16", "x3", "f32")                                         # the fp8 / fp16 kernels take batch == 1 only
FAMILIES = ("bf16", "x3", "fp8", "fp16", "f32")


def tiled_tiles(ops, fam):
    if fam == "bf16":
        return [-1] + [c for c in ops._TILE_CANDIDATES if c not in APANEL["bf16"]]
    if fam == "x3":
        return [-1] + list(ops._X3_CANDIDATES)
    if fam == "fp8":
        return [-1] + list(ops._LOWP_CANDIDATES)
    return {"fp16": [-1, 0, 1, 2], "f32": [-1, 0, 1, 2, 3]}[fam]


def panel_candidates(ops, fam):
    lists = (ops._TILE_CANDIDATES, ops._A_LN_CANDIDATES) if fam == "bf16" else (ops._A_LN_X3_CANDIDATES,)
    return sorted({t for l in lists for t in l if t in APANEL[fam]})


def ldc_min_above(N, odt):
    """The smallest legal leading dimension above N: N + 1, or the next multiple of 8 for split-fp16 rows (header: ld % 8)."""
    return (N // 8 + 1) * 8 if odt == H2 else N + 1


class Case:
    def __init__(self, name, M, N, ldc, act=0, bias=None, alpha=1.0, residual=False, inplace=False, batch=1, gap=0, tags=()):
        self.name, self.M, self.N, self.ldc, self.act, self.bias, self.alpha = name, M, N, ldc, act, bias, alpha
        self.residual, self.inplace, self.batch, self.gap, self.tags = residual, inplace, batch, gap, set(tags)


def cases(fam, bm, odt):
    """Ragged M (M % 16 in {1, 8, 9}, one short of / one over the tile height), ragged N (N % 64, N % 8, odd), N % 64 == 0
    (whole-line stores), ldc in {smallest legal step above N, N + 8, N + 64, N rounded up to 64 and to 32}, batched with
    strideC > M·ldc and a per-row bias, and every epilogue."""
    out = [Case("short-M plain ldc=N+8", bm - 1, 200, 208, tags=("raggedM", "raggedN", "ldc")),
           Case("over-M odd-N bias+relu ldc=min", bm + 1, 197, ldc_min_above(197, odt), act=2, bias="col",
                tags=("raggedM", "raggedN", "ldc")),
           Case("M%16=8 N%64=0 bias+gelu ldc=N+64", 40, 192, 256, act=1, bias="col", tags=("raggedM", "ldc"))]
    if odt == FP8:           # (an fp8 output takes no residual: ODIC_EINVAL)
        out.append(Case("M%16=9 odd-N alpha+bias ldc=up64", 41, 203, 256, bias="col", alpha=0.5, tags=("raggedM", "raggedN", "ldc")))
    else:
        out.append(Case("M%16=9 odd-N alpha+bias+residual(ldr>N) ldc=up64", 41, 203, 256, bias="col", alpha=0.5, residual=True,
                        tags=("raggedM", "raggedN", "ldc")))
    if fam in BATCHED:
        out.append(Case("batched strideC>M*ldc row-bias sigmoid ldc=up32", bm - 1, 100, 128, act=3, bias="row", batch=3, gap=24,
                        tags=("raggedM", "raggedN", "ldc")))
    else:
        out.append(Case("row-bias sigmoid ldc=up32", bm - 1, 100, 128, act=3, bias="row", tags=("raggedM", "raggedN", "ldc")))
    if odt == F32:
        out.append(Case("in-place residual (out = residual) ldc=ldr=N+64", bm + 1, 192, 256, bias="col", residual=True, inplace=True,
                        tags=("raggedM", "ldc")))
    return out




def panel_cases(fam, tile, odt):
    """The A-resident tiles take whole tiles only (ragged M / N are refused): ldc > N, the residual forms."""
    bm, bnc, K = APANEL[fam][tile]
    M, N = 2 * bm, 3 * bnc
    out = [Case("plain ldc=N+8", M, N, N + 8, tags=("ldc",)),
           Case("bias+gelu ldc=N+64", M, N, N + 64, act=1, bias="col", tags=("ldc",))]
    if odt == F32 and fam == "bf16" and tile != 50:          # (the 64-row-per-wave form has no residual instantiation)
        out += [Case("alpha+bias+residual ldc=up64", M, N, -(-(N + 1) // 64) * 64, bias="col", alpha=0.5, residual=True, tags=("ldc",)),
                Case("in-place residual", M, N, N + 64, bias="col", residual=True, inplace=True, tags=("ldc",))]
    return out
