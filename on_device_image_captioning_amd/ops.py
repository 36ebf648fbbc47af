"""Thin torch-tensor wrappers over the C ABI (include/odic_hip.h).

PyTorch is plumbing here: tensors own device memory and the current stream; every function hands
`data_ptr()`s and sizes to libodic_hip.so.  Nothing in this module computes on the CPU and nothing
falls back — a non-CUDA tensor or a missing library raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch

from . import _hip
from ._hip import ACT_GELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, BF16, F16, F32, FP8, H2  # noqa: F401  (re-exported)

FP8_DTYPE = torch.float8_e4m3fn          # OCP e4m3: the fp8 format of gfx950's MFMA
FP8_MAX = 448.0
# Split-fp16 tensors (ODIC_H2: hi + lo fp16 pairs, 4 bytes per element in [8 hi | 8 lo] groups — include/odic_hip.h)
# travel as torch.int32 tensors of the LOGICAL shape: same sizes, strides and zero bytes as the fp32 tensor they
# replace, and a dtype no other operand of this library uses.
H2_DTYPE = torch.int32
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, FP8_DTYPE: FP8, H2_DTYPE: H2}


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py's roofline pass): HIP events recorded on the launch stream
# around every C-ABI call, tagged with the kernel family and its algorithmic FLOPs / bytes.
# ----------------------------------------------------------------------------------------------
_PROFILE: Optional[list] = None


class profile:
    """`with ops.profile() as recs:` → recs = [(family, flops, bytes, start_evt, end_evt, detail), ...]"""

    def __enter__(self):
        global _PROFILE
        _PROFILE = []
        return _PROFILE

    def __exit__(self, *exc):
        global _PROFILE
        _PROFILE = None
        return False


class _timed:
    __slots__ = ("family", "flops", "bytes", "start", "detail")

    def __init__(self, family: str, flops: float, nbytes: float, detail: str = ""):
        self.family, self.flops, self.bytes, self.start, self.detail = family, flops, nbytes, None, detail

    def __enter__(self):
        if _PROFILE is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if self.start is not None:
            end = torch.cuda.Event(enable_timing=True)
            end.record()
            _PROFILE.append((self.family, self.flops, self.bytes, self.start, end, self.detail))
        return False


#: position index of the decoder step being launched, set by the host loop while a profile is active
#: (the kernels read *pos from device memory; the host needs it only to price the step's cache reads)
_STEP_T: Optional[int] = None


def set_step_hint(t: Optional[int]) -> None:
    global _STEP_T
    _STEP_T = t


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("odic ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DT[dt]
    except KeyError:
        raise RuntimeError(f"unsupported dtype {dt}") from None


# ----------------------------------------------------------------------------------------------
# bf16 GEMM tile autotuning: "measure, don't guess".  While `autotune()` is active (the eager warm-up
# pass of a pipeline, never inside a stream capture) the first call of every distinct problem shape
# times the candidate tile configurations with HIP events on scratch outputs and remembers the
# fastest; later calls (including the captured ones) reuse the choice.
_TILE_CHOICE: dict = {}
_TUNING = False
# ODIC_TILE_CACHE=<file>: tile choices are loaded from / appended to a JSON file, so a later process (a profiler
# pass that must not contain tuning launches, a server restart) starts from the measured choices
_TILE_CACHE_FILE = os.environ.get("ODIC_TILE_CACHE")


def _cache_key(key) -> str:
    return "|".join(str(k) for k in key)


def _load_tile_cache() -> dict:
    if _TILE_CACHE_FILE and os.path.exists(_TILE_CACHE_FILE):
        import json
        with open(_TILE_CACHE_FILE) as f:
            return json.load(f)
    return {}


_TILE_CACHE: dict = _load_tile_cache()
_TILE_CANDIDATES = tuple(int(c) for c in os.environ.get("ODIC_TILE_CANDIDATES", "0,1,7,10,40,41,42,50,51,52,53").split(","))


class autotune:
    def __enter__(self):
        global _TUNING
        self._prev, _TUNING = _TUNING, True
        return _TILE_CHOICE

    def __exit__(self, *exc):
        global _TUNING
        _TUNING = self._prev
        return False


_LOWP_CANDIDATES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)   # gemm_lowp.hip tile configurations (fp8 / fp16 operands; 5-9: the
                                                    # block-scaled fp8 MFMA, rejected for fp16 / K % 128 != 0 and then skipped)
_X3_CANDIDATES = tuple(int(c) for c in os.environ.get("ODIC_X3_TILE_CANDIDATES", "0,1,2,5,6,7,8").split(","))   # gemm_x3.hip


def _tile_choice(key, tile_cfg: int) -> Optional[int]:
    """The caller's explicit `tile_cfg`, else the choice this process remembers for `key`, else the one the ODIC_TILE_CACHE
    file holds (remembered from then on); None when the shape has no choice yet."""
    if tile_cfg >= 0:
        return tile_cfg
    cfg = _TILE_CHOICE.get(key)
    if cfg is None and _TILE_CACHE:
        cfg = _TILE_CACHE.get(_cache_key(key))
        if cfg is not None:
            _TILE_CHOICE[key] = cfg
    return cfg


def _tune_gemm(args: "_hip.GemmArgs", key, out: torch.Tensor, candidates=None) -> int:
    lib = _hip.load()
    scratch = torch.empty_like(out)
    real_out = args.out
    args.out = scratch.data_ptr()
    best, best_ms = -1, float("inf")
    try:
        for cfg in (candidates or _TILE_CANDIDATES):
            args.tile_cfg = cfg
            if lib.odic_gemm(C.byref(args), _stream()) != 0:
                continue
            lib.odic_gemm(C.byref(args), _stream())
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(4):
                lib.odic_gemm(C.byref(args), _stream())
            en.record()
            en.synchronize()
            ms = st.elapsed_time(en)
            if ms < best_ms:
                best, best_ms = cfg, ms
    finally:
        args.out = real_out
    _TILE_CHOICE[key] = best
    if _TILE_CACHE_FILE:
        import json
        _TILE_CACHE[_cache_key(key)] = best
        with open(_TILE_CACHE_FILE, "w") as f:
            json.dump(_TILE_CACHE, f, indent=0)
    return best


def row_view(t: torch.Tensor, what: str, batch: int = 1) -> tuple:
    """(rows, width, leading dimension, batch stride) of one operand view, from its shape and strides alone.
    A 2-D view with unit column stride keeps its row stride; any other tensor must be contiguous and is flattened to
    [numel / width, width].  batch > 1: a 3-D view [batch, rows, width] carries its own batch stride, a 2-D view is
    shared by all batches (batch stride 0)."""
    shape, stride = t.shape, t.stride()         # (read once: this runs for every operand of every decoder-step product)
    nd, bs = len(shape), 0
    if batch > 1 and nd != 2:
        if nd != 3 or shape[0] != batch:
            raise RuntimeError(f"{what}: a batched operand is [batch={batch}, rows, cols] or a shared 2-D view, "
                               f"got {tuple(shape)}")
        nd, bs = 2, stride[0]
    width = shape[-1]
    if nd == 2:
        ld = stride[-2]
        if stride[-1] == 1 and ld >= width:
            return shape[-2], width, ld, bs
        if batch > 1 or not t.is_contiguous():
            raise RuntimeError(f"{what}: column stride {stride[-1]} (must be 1)" if stride[-1] != 1 else
                               f"{what}: row stride {ld} is smaller than the row width {width}")
    elif not t.is_contiguous():
        raise RuntimeError(f"{what}: a view of {nd} dimensions must be contiguous")
    return t.numel() // width, width, width, 0


def gemm_dims(A: torch.Tensor, W: torch.Tensor, residual: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None, batch: int = 1) -> tuple:
    """(M, N, K, lda, ldw, ldr, ldc, batch, strideA, strideW, strideR, strideC) of out = A·Wᵀ (+ residual), read off the
    views: every operand has unit column stride, A is [M, K] and W [N, K]; `out` and `residual` have at least N columns
    (only the first N are the product's, the row stride is the leading dimension).  batch == 1: 2-D row-strided views,
    or contiguous tensors of any rank flattened to rows.  batch > 1: 3-D views [batch, rows, cols] and shared 2-D views,
    `out` always 3-D.  Reads shapes and strides only (CPU tensors do); raises RuntimeError on what a view cannot say."""
    M, K, lda, sA = row_view(A, "gemm A", batch)
    N, Kw, ldw, sW = row_view(W, "gemm W", batch)
    if Kw != K:
        raise RuntimeError(f"gemm: A has K = {K} columns, W has {Kw}")
    ldr = sR = sC = 0
    ldc = N
    if out is not None:
        if batch > 1 and out.dim() != 3:
            raise RuntimeError("gemm: the `out` of a batched product is [batch, rows, cols]")
        Mo, No, ldc, sC = row_view(out, "gemm out", batch)
        if No < N or Mo < M:
            raise RuntimeError(f"gemm: out [{Mo}, {No}] does not hold the [{M}, {N}] product")
    elif batch > 1:
        raise RuntimeError("gemm: a batched product with implicit shapes needs `out`")
    if residual is not None and residual is out:        # in place on a residual stream: read once
        ldr, sR = ldc, sC
    elif residual is not None:
        Mr, Nr, ldr, sR = row_view(residual, "gemm residual", batch)
        if Nr < N or Mr < M:
            raise RuntimeError(f"gemm: residual [{Mr}, {Nr}] does not hold the [{M}, {N}] product")
    return M, N, K, lda, ldw, ldr, ldc, batch, sA, sW, sR, sC


def gemm(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor] = None,
         residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, *, act: int = ACT_NONE,
         alpha: float = 1.0, bias_axis: int = 0, out_dtype: Optional[torch.dtype] = None,
         M: Optional[int] = None, N: Optional[int] = None, K: Optional[int] = None,
         lda: Optional[int] = None, ldw: Optional[int] = None, ldr: Optional[int] = None,
         ldc: Optional[int] = None, batch: int = 1, strideA: int = 0, strideW: int = 0, strideBias: int = 0,
         strideR: int = 0, strideC: int = 0, ln_fold: Optional[tuple] = None, tile_cfg: int = -1,
         col_scale: Optional[torch.Tensor] = None, out_scale: float = 1.0,
         a_ln: Optional[torch.Tensor] = None, ln_eps: float = 1e-5, dims: Optional[tuple] = None) -> torch.Tensor:
    """out = act(alpha·A·Wᵀ + bias) + residual.  With no explicit M, every dimension, leading dimension and batch
    stride is read off the views (gemm_dims): unit column stride, A [M,K] and W [N,K] of exactly the operand's width,
    `out` / `residual` possibly wider than N (a slice of a wider buffer); contiguous tensors of any rank are flattened
    to rows; with `batch` > 1 the operands are [batch, rows, cols] views or shared 2-D ones.  `dims`: what gemm_dims
    returned for operands of these shapes and strides, kept by a call site that runs every decoder step.  Explicit
    dims / leading dimensions / batch strides (elements) are taken as given instead, and only together with M.
    ln_fold = (colsum, eps): W and bias come from fold_layernorm() and
    the rows of A are LayerNorm-ed inside the product (fp32 skinny-M path only).  fp8 / fp16 operands (the
    low-precision backbone mode): `col_scale` fp32 [N] multiplies column n of A·Wᵀ (activation scale x weight channel
    scale) and `out_scale` the result before an fp8 / fp16 output cast.
    LayerNorm while reading (A = None, `a_ln` = the fp32 rows [M,K], W / bias from fold_layernorm_bf16()): the bf16
    A-resident kernels normalise each row in registers — one launch for norm → linear (K = 192 / 384, whole tiles)."""
    if a_ln is not None:
        return _gemm_a_ln(a_ln, W, bias, out, act=act, alpha=alpha, out_dtype=out_dtype, ln_eps=ln_eps, tile_cfg=tile_cfg)
    if M is None and (not (N is K is lda is ldw is ldr is ldc is None) or strideA or strideW or strideR or strideC):
        raise RuntimeError("gemm: N / K / leading dimensions / batch strides are explicit only together with M")
    _need_cuda(A, W, bias, residual, out, col_scale)
    if A.dtype != W.dtype:
        raise RuntimeError("A and W must share a dtype")
    if dims is not None:
        M, N, K, lda, ldw, ldr, ldc, batch, strideA, strideW, strideR, strideC = dims
    elif M is None:
        M, N, K, lda, ldw, ldr, ldc, batch, strideA, strideW, strideR, strideC = gemm_dims(A, W, residual, out, batch)
    odt = out_dtype or (out.dtype if out is not None else A.dtype)
    if out is None:
        out = torch.empty((batch, M, N) if batch > 1 else (*A.shape[:-1], N), dtype=odt, device=A.device)
        if ldc is None:
            ldc = N
        if batch > 1 and strideC == 0:
            strideC = M * N
    if ldc is None:
        ldc = N
    if residual is not None and ldr is None:
        ldr = N
    if bias is not None and bias.dtype != torch.float32:
        raise RuntimeError("bias must be fp32")
    if residual is not None and residual.dtype != torch.float32:
        raise RuntimeError("residual must be fp32")
    a = _hip.GemmArgs(_p(A), _p(W), _p(bias), _p(residual), _p(out), M, N, K, lda, ldw, ldr or 0, ldc, batch,
                      strideA, strideW, strideBias, strideR, strideC, alpha, act, bias_axis,
                      dtype_code(A.dtype), dtype_code(out.dtype), tile_cfg,
                      _p(ln_fold[0]) if ln_fold else None, float(ln_fold[1]) if ln_fold else 0.0, None,
                      _p(col_scale), float(out_scale), None, 0, None, None)
    if A.dtype in (torch.bfloat16, torch.float16, FP8_DTYPE, H2_DTYPE):
        key = (A.dtype, M, N, K, batch, out.dtype, act, residual is not None)
        cfg = _tile_choice(key, tile_cfg)
        if cfg is None and _TUNING and _PROFILE is None and ldc == N and batch == 1 \
                and not torch.cuda.is_current_stream_capturing():
            cfg = _tune_gemm(a, key, out, None if A.dtype == torch.bfloat16 else
                             (_X3_CANDIDATES if A.dtype == H2_DTYPE else _LOWP_CANDIDATES))
        if cfg is not None:
            a.tile_cfg = cfg
    isz, osz = A.element_size(), out.element_size()
    nbytes = batch * ((M * K if strideA or batch == 1 else M * K / batch) * isz +
                      (N * K if strideW or batch == 1 else N * K / batch) * isz + M * N * osz +
                      (M * N * 4 if residual is not None else 0))
    fam = {torch.bfloat16: "gemm_bf16", torch.float16: "gemm_f16", FP8_DTYPE: "gemm_fp8",
           H2_DTYPE: "gemm_x3"}.get(A.dtype, "gemm_f32")
    with _timed(fam, 2.0 * M * N * K * batch, nbytes,
                f"{M}x{N}x{K}" + (f"x{batch}" if batch > 1 else "")):
        _hip.check(_hip.load().odic_gemm(C.byref(a), _stream()), "odic_gemm")
    return out


_A_LN_CANDIDATES = (50, 52, 51, 53)          # the A-resident tile configurations (gemm_bf16_apanel_kernel)
_A_LN_X3_CANDIDATES = (20, 21)               # gemm_x3_apanel_kernel (K = 192)


def _gemm_a_ln(x: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], out: Optional[torch.Tensor], *, act: int,
               alpha: float, out_dtype: Optional[torch.dtype], ln_eps: float, tile_cfg: int) -> torch.Tensor:
    """out = act(alpha·LN0(x)·Wᵀ + bias), LN0 = LayerNorm without affine, computed while the fp32 rows are read
    (odic_gemm_args.a_ln).  x fp32 [M,K] contiguous, W bf16 [N,K] contiguous."""
    _need_cuda(x, W, bias, out)
    if x.dtype != torch.float32 or W.dtype not in (torch.bfloat16, H2_DTYPE) or not (x.is_contiguous() and W.is_contiguous()):
        raise RuntimeError("gemm(a_ln=...): contiguous fp32 rows and a contiguous bf16 / split-fp16 weight")
    K = x.shape[-1]
    M, N = x.numel() // K, W.shape[0]
    if out is None:
        out = torch.empty(*x.shape[:-1], N, dtype=out_dtype or W.dtype, device=x.device)
    a = _hip.GemmArgs(None, _p(W), _p(bias), None, _p(out), M, N, K, K, K, 0, N, 1, 0, 0, 0, 0, 0, alpha, act, 0,
                      dtype_code(W.dtype), dtype_code(out.dtype), tile_cfg, None, float(ln_eps), None, None, 1.0, None, 0, None, None,
                      _p(x), K)
    key = ("a_ln", W.dtype, M, N, K, out.dtype, act)
    cfg = _tile_choice(key, tile_cfg)
    if cfg is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("gemm(a_ln=...): no tile choice for this shape yet — run it once outside graph capture")
        cfg = _tune_gemm(a, key, out, _A_LN_CANDIDATES if W.dtype == torch.bfloat16 else _A_LN_X3_CANDIDATES)
        if cfg < 0:
            raise RuntimeError(f"gemm(a_ln=...): no A-resident tile configuration takes {M}x{N}x{K}")
    a.tile_cfg = cfg
    with _timed("gemm_bf16" if W.dtype == torch.bfloat16 else "gemm_x3", 2.0 * M * N * K,
                M * K * 4 + N * K * W.element_size() + M * N * out.element_size(), f"ln+{M}x{N}x{K}"):
        _hip.check(_hip.load().odic_gemm(C.byref(a), _stream()), "odic_gemm")
    return out


def a_ln_supported(M: int, N: int, K: int, dtype=torch.bfloat16) -> bool:
    """Shapes the LayerNorm-while-reading form takes: K = 192 (128-row panels, 64-column chunks) or 384 (128 / 32); split
    fp16: K = 192 (64-row panels, 32-column chunks)."""
    if dtype == H2_DTYPE:
        return K == 192 and M % 64 == 0 and N % 32 == 0
    return (K == 192 and M % 128 == 0 and N % 64 == 0) or (K == 384 and M % 128 == 0 and N % 32 == 0)


def fold_layernorm(W: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """Weight-pack-time half of odic_gemm's folded LayerNorm: (W·diag(gamma), bias + W·beta, row sums of
    W·diag(gamma)), all fp32, computed in fp64.  LayerNorm(a)·Wᵀ + bias = rstd·(a·W'ᵀ − mean·colsum) + bias'."""
    W64 = W.double()
    Wg = W64 * gamma.double()[None, :]
    b2 = W64 @ beta.double() + (bias.double() if bias is not None else 0.0)
    return Wg.float().contiguous(), b2.float().contiguous(), Wg.sum(1).float().contiguous()


def fold_layernorm_bf16(W: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """Weight-pack-time half of the LayerNorm folded across two bf16 products: (bf16 W·diag(gamma), fp32 bias + W·beta,
    fp32 row sums of the ROUNDED bf16 weights — the kernel subtracts mean·colsum from a product of exactly those)."""
    Wg, b2, _ = fold_layernorm(W, bias, gamma, beta)
    W16 = Wg.to(torch.bfloat16).contiguous()
    return W16, b2, W16.double().sum(1).float().contiguous()


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, *, eps: float = 1e-5,
              out_dtype: torch.dtype = torch.float32, out: Optional[torch.Tensor] = None,
              M: Optional[int] = None, C_: Optional[int] = None, ldx: Optional[int] = None) -> torch.Tensor:
    _need_cuda(x, gamma, beta, out)
    if M is None:
        M, C_, ldx, _ = row_view(x, "layernorm input")
    if out is None:
        out = torch.empty((M, C_) if x.dim() < 2 or ldx != C_ else x.shape, dtype=out_dtype, device=x.device)
    with _timed("layernorm", 8.0 * M * C_, M * C_ * (4 + out.element_size())):
        _hip.check(_hip.load().odic_layernorm(_p(x), ldx, _p(gamma), _p(beta), _p(out), M, C_, eps,
                                              dtype_code(out.dtype), _stream()), "odic_layernorm")
    return out


def _cast(x: torch.Tensor, M: Optional[int], C_: Optional[int], ldx: Optional[int], dtype: torch.dtype, to: str,
          nbytes: float) -> torch.Tensor:
    """fp32 [M,C] (row stride ldx; with no explicit M: a 2-D row-strided view or a contiguous tensor) → contiguous [M,C]."""
    _need_cuda(x)
    if M is None:
        M, C_, ldx, _ = row_view(x, "cast_" + to + " input")
    out = torch.empty((M, C_), dtype=dtype, device=x.device)
    with _timed("cast_" + to, 0.0, M * C_ * nbytes):
        _hip.check(getattr(_hip.load(), "odic_cast_f32_to_" + to)(_p(x), ldx, _p(out), C_, M, C_, _stream()),
                   "odic_cast_f32_to_" + to)
    return out


def cast_bf16(x: torch.Tensor, *, M: Optional[int] = None, C_: Optional[int] = None, ldx: Optional[int] = None
              ) -> torch.Tensor:
    """fp32 [M,C] (row stride ldx) → contiguous bf16 [M,C]."""
    return _cast(x, M, C_, ldx, torch.bfloat16, "bf16", 6.0)


def cast_h2(x: torch.Tensor, *, M: Optional[int] = None, C_: Optional[int] = None, ldx: Optional[int] = None
            ) -> torch.Tensor:
    """fp32 [M,C] (row stride ldx) → contiguous split-fp16 [M,C] (an int32 tensor, see H2_DTYPE)."""
    return _cast(x, M, C_, ldx, H2_DTYPE, "h2", 8.0)


def h2_from_f32(x: torch.Tensor) -> torch.Tensor:
    """Weight-pack-time split of an fp32 tensor [..., K] (K % 8 == 0) into the h2 layout, on the tensor's device with
    plain torch ops (exact: two round-to-nearest-even fp16 conversions).  The bits the device writes, NaN payloads aside
    (csrc/odic_common.h::h2_split): |x| > 65504 and ±inf saturate to ±65504, a NaN leaves as hi = lo = NaN."""
    if x.shape[-1] % 8:
        raise RuntimeError("h2 rows are whole groups of 8 elements")
    x = x.detach().float().clamp(-65504.0, 65504.0)         # (torch.clamp keeps a NaN)
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    g = torch.stack([hi.reshape(*x.shape[:-1], -1, 8), lo.reshape(*x.shape[:-1], -1, 8)], dim=-2)   # [..., K/8, 2, 8]
    return g.contiguous().view(torch.int32).reshape(x.shape)


def h2_to_f32(t: torch.Tensor) -> torch.Tensor:
    """Inverse of h2_from_f32 (tests, taps): hi + lo in fp32."""
    g = t.contiguous().view(torch.float16).reshape(*t.shape[:-1], -1, 2, 8).float()
    return (g[..., 0, :] + g[..., 1, :]).reshape(t.shape)


def pow2_scale_for_h2(w: torch.Tensor) -> float:
    """Power of two s such that max|w|·s lies in [2^12, 2^13): the hi parts sit far from the fp16 overflow and the lo
    parts (|lo| <= |w|·s·2^-11) of all but negligible elements stay fp16 normals.  Exact to undo (alpha = 1/s)."""
    import math
    m = float(w.detach().abs().max())
    if not (m > 0.0) or not math.isfinite(m):
        return 1.0
    return float(2.0 ** (12 - math.floor(math.log2(m))))


def copy(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst ← src (contiguous, same shape and dtype, a multiple of 16 bytes) by a kernel of this library."""
    _need_cuda(src, dst)
    if src.shape != dst.shape or src.dtype != dst.dtype or not src.is_contiguous() or not dst.is_contiguous():
        raise RuntimeError("copy: contiguous tensors of one shape and dtype expected")
    nbytes = src.numel() * src.element_size()
    with _timed("copy", 0.0, 2.0 * nbytes):
        _hip.check(_hip.load().odic_copy(_p(src), _p(dst), nbytes, _stream()), "odic_copy")
    return dst


def patch_merge_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, B: int, res: int, Cin: int,
                          *, eps: float = 1e-5, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    _need_cuda(x, gamma, beta)
    out = torch.empty((B, (res // 2) ** 2, 4 * Cin), dtype=out_dtype, device=x.device)
    with _timed("patch_merge_layernorm", 8.0 * out.numel(), out.numel() * (4 + out.element_size())):
        _hip.check(_hip.load().odic_patch_merge_layernorm(_p(x), _p(gamma), _p(beta), _p(out), B, res, Cin, eps,
                                                          dtype_code(out_dtype), _stream()),
                   "odic_patch_merge_layernorm")
    return out


def patch_embed(img: torch.Tensor, w: torch.Tensor, b: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
                patch: int, *, eps: float = 1e-5) -> torch.Tensor:
    _need_cuda(img, w, b, gamma, beta)
    B, Cin, H, Wd = img.shape
    Cout = w.shape[0]
    if not img.is_contiguous() or img.dtype != torch.float32:
        raise RuntimeError("patch_embed: image batch must be contiguous fp32 [B,C,H,W]")
    out = torch.empty((B, (H // patch) * (Wd // patch), Cout), dtype=torch.float32, device=img.device)
    with _timed("patch_embed", 2.0 * out.numel() * Cin * patch * patch, (img.numel() + out.numel()) * 4):
        _hip.check(_hip.load().odic_patch_embed(_p(img), _p(w), _p(b), _p(gamma), _p(beta), _p(out), B, Cin, H, Wd,
                                                patch, Cout, eps, _stream()), "odic_patch_embed")
    return out


def shifted_bias_prescaled(bias_table: torch.Tensor, ws: int, scale: float) -> torch.Tensor:
    """[heads, 4, 576] fp32 — weight-pack-time plumbing for odic_window_attention's fast path (ws = 12): the
    relative-position bias table (reference swin_transformer_mod.py:163-173,196-198) with its x axis reversed and
    rows padded to 24, divided by `scale`, in four copies shifted by 0..3 floats, so that the biases of the four
    consecutive keys of an MFMA accumulator quad are one aligned 16-byte LDS read (include/odic_hip.h)."""
    if ws != 12:
        raise RuntimeError("the packed bias layout is specialised for 12x12 windows")
    heads = bias_table.shape[1]
    t = (bias_table.double() / scale).float().view(23, 23, heads)           # [r, c, head]
    R = torch.zeros(heads, 23 * 24 + 32, dtype=torch.float32, device=bias_table.device)
    R[:, :23 * 24].view(heads, 23, 24)[:, :, :23] = t.flip(1).permute(2, 0, 1)
    out = torch.zeros(heads, 4, 576, dtype=torch.float32, device=bias_table.device)
    for s_ in range(4):
        out[:, s_, :] = R[:, s_:s_ + 576]
    return out.contiguous()


def swin_qkv_attention(x: torch.Tensor, w_folded: torch.Tensor, b_folded: torch.Tensor, bias_shifted_prescaled: torch.Tensor,
                       B: int, res: int, C_: int, heads: int, ws: int, shift: int, *, eps: float = 1e-5,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """norm1 → qkv → attention core in one launch (odic_swin_qkv_attention; width 192, ws 12).  x fp32 [B·res², C] contiguous,
    (w_folded, b_folded) from fold_layernorm_bf16(qkv.weight, qkv.bias, norm1.weight, norm1.bias) → bf16 [B·res², C]."""
    _need_cuda(x, w_folded, b_folded, bias_shifted_prescaled, out)
    if x.dtype != torch.float32 or w_folded.dtype != torch.bfloat16 or not (x.is_contiguous() and w_folded.is_contiguous()):
        raise RuntimeError("swin_qkv_attention: contiguous fp32 rows and a contiguous bf16 folded weight")
    if out is None:
        out = torch.empty(B * res * res, C_, dtype=torch.bfloat16, device=x.device)
    nwh = B * (res // ws) ** 2 * heads
    with _timed("swin_qkv_attention", 2.0 * B * res * res * C_ * 3 * C_ + nwh * 2654208.0,
                B * res * res * C_ * (4 + 2) + 3 * C_ * C_ * 2, f"res{res}h{heads}"):
        _hip.check(_hip.load().odic_swin_qkv_attention(_p(x), C_, _p(w_folded), _p(b_folded), _p(bias_shifted_prescaled),
                                                      _p(out), B, res, C_, heads, ws, shift, (C_ // heads) ** -0.5, eps,
                                                      _stream()), "odic_swin_qkv_attention")
    return out


def swin_qkv_attention_tiled_supported(M: int, C_: int, heads: int, ws: int, res: int, dtype=torch.bfloat16) -> bool:
    """Shapes odic_swin_qkv_attention_tiled takes: bf16, 12 x 12 windows, head dim 32, heads in threes, width a multiple
    of 64, whole windows.  (One tile form, chosen by this rule and not by a timed run: the call is legal inside a stream
    capture at a shape never run before.)"""
    return (dtype == torch.bfloat16 and ws == 12 and heads > 0 and heads * 32 == C_ and heads % 3 == 0 and C_ % 64 == 0
            and res > 0 and res % ws == 0 and M > 0 and M % (res * res) == 0)


def swin_qkv_attention_tiled(xn: torch.Tensor, w_qkv: torch.Tensor, b_qkv: torch.Tensor, bias_shifted_prescaled: torch.Tensor,
                             B: int, res: int, C_: int, heads: int, ws: int, shift: int, *,
                             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv → attention core in one launch (odic_swin_qkv_attention_tiled; widths 384 / 768 / 1536, ws 12).  xn bf16
    [B·res², C] contiguous (the norm1 output), w_qkv bf16 [3C, C] contiguous, b_qkv fp32 [3C] → bf16 [B·res², C]."""
    _need_cuda(xn, w_qkv, b_qkv, bias_shifted_prescaled, out)
    if (xn.dtype != torch.bfloat16 or w_qkv.dtype != torch.bfloat16 or not (xn.is_contiguous() and w_qkv.is_contiguous())
            or xn.numel() != B * res * res * C_ or w_qkv.numel() != 3 * C_ * C_):
        raise RuntimeError("swin_qkv_attention_tiled: contiguous bf16 rows [B·res², C] and a contiguous bf16 weight [3C, C]")
    if out is None:
        out = torch.empty(B * res * res, C_, dtype=torch.bfloat16, device=xn.device)
    nwh = B * (res // ws) ** 2 * heads if ws > 0 else 0
    with _timed("swin_qkv_attention", 2.0 * B * res * res * C_ * 3 * C_ + nwh * 2654208.0,
                B * res * res * C_ * (2 + 2) + 3 * C_ * C_ * 2 + 3 * C_ * 4 + heads * 9216, f"res{res}h{heads}"):
        _hip.check(_hip.load().odic_swin_qkv_attention_tiled(_p(xn), _p(w_qkv), _p(b_qkv), _p(bias_shifted_prescaled), _p(out),
                                                            B, res, C_, heads, ws, shift, (C_ // heads) ** -0.5 if heads > 0 else 0.0,
                                                            _stream()), "odic_swin_qkv_attention_tiled")
    return out


def swin_mlp_supported(M: int, C_: int, dtype=torch.bfloat16) -> bool:
    """Shapes odic_swin_mlp takes: bf16 weights, width 192, whole 128-row panels.  (One tile form, chosen by this rule
    and not by a timed run: the call is legal inside a stream capture at a shape never run before.)"""
    return dtype == torch.bfloat16 and C_ == 192 and M > 0 and M % 128 == 0


def swin_mlp(x: torch.Tensor, w1_folded: torch.Tensor, b1_folded: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor,
             alpha2: float = 1.0, out: Optional[torch.Tensor] = None, ln_eps: float = 1e-5) -> torch.Tensor:
    """x + fc2(GELU(fc1(LN0(x)))) in one launch (odic_swin_mlp; width 192): the bf16 hidden activations stay in registers.
    x fp32 [M, C] contiguous, (w1_folded, b1_folded) from fold_layernorm_bf16(fc1.weight, fc1.bias, norm2.weight,
    norm2.bias), w2 bf16 [C, 4C] with its fp32 bias and alpha.  `out` may be x itself (in place).  Bit-identical to
    gemm(None, w1_folded, b1_folded, a_ln=x, act=ACT_GELU) followed by gemm(h, w2, b2, residual=x, alpha=alpha2)."""
    _need_cuda(x, w1_folded, b1_folded, w2, b2, out)
    if x.dtype != torch.float32 or w1_folded.dtype != torch.bfloat16 or w2.dtype != torch.bfloat16 or \
            not (x.is_contiguous() and w1_folded.is_contiguous() and w2.is_contiguous()):
        raise RuntimeError("swin_mlp: contiguous fp32 rows and contiguous bf16 weights")
    C_ = x.shape[-1]
    M = x.numel() // C_
    if tuple(w1_folded.shape) != (4 * C_, C_) or tuple(w2.shape) != (C_, 4 * C_) or b1_folded.numel() != 4 * C_ or \
            b2.numel() != C_ or b1_folded.dtype != torch.float32 or b2.dtype != torch.float32:
        raise RuntimeError("swin_mlp: fc1 is [4C, C] with an fp32 bias [4C], fc2 [C, 4C] with an fp32 bias [C]")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous():
        raise RuntimeError("swin_mlp: out is a contiguous fp32 tensor of x's shape")
    with _timed("swin_mlp", 2.0 * M * C_ * 4 * C_ * 2, 2.0 * M * C_ * 4 + 2 * 4 * C_ * C_ * 2, f"{M}x{C_}"):
        _hip.check(_hip.load().odic_swin_mlp(_p(x), C_, _p(w1_folded), _p(b1_folded), _p(w2), _p(b2), float(alpha2), _p(out),
                                             C_, M, C_, float(ln_eps), _stream()), "odic_swin_mlp")
    return out


def window_attention(qkv: torch.Tensor, bias_table: torch.Tensor, B: int, res: int, C_: int, heads: int, ws: int,
                     shift: int, *, scale: Optional[float] = None, out: Optional[torch.Tensor] = None,
                     bias_shifted_prescaled: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`bias_shifted_prescaled` must have been packed with the same `scale` (default head_dim^-0.5)."""
    _need_cuda(qkv, bias_table, out, bias_shifted_prescaled)
    if scale is None:
        scale = (C_ // heads) ** -0.5
    if out is None:
        out = torch.empty((B * res * res, C_), dtype=qkv.dtype, device=qkv.device)
    # algorithmic work per (window, head): QKᵀ + PV = 4·N²·hd FLOP; q,k,v in + o out = 4·N·hd elements
    inst = B * (res // ws) ** 2 * heads
    n = ws * ws
    fam = ("window_attention_bf16" if qkv.dtype in (torch.bfloat16, torch.float16) else
           "window_attention_x3" if qkv.dtype == H2_DTYPE else "window_attention_f32")
    with _timed(fam, inst * 4.0 * n * n * 32, inst * 4.0 * n * 32 * qkv.element_size(), f"res{res}h{heads}"):
        _hip.check(_hip.load().odic_window_attention(_p(qkv), _p(bias_table), _p(bias_shifted_prescaled), _p(out), B, res, C_,
                                                     heads, ws, shift,
                                                     scale, dtype_code(qkv.dtype), _stream()),
                   "odic_window_attention")
    return out


# ----------------------------------------------------------------------------------------------
def stcexp_group_meta(groups: Sequence[int], device) -> torch.Tensor:
    starts = [0]
    gid = []
    for g, n in enumerate(groups):
        starts.append(starts[-1] + n)
        gid += [g] * n
    return torch.tensor(starts + gid, dtype=torch.int32, device=device)


def stcexp_normalize(z: torch.Tensor, enc_len: torch.Tensor, group_meta: torch.Tensor, ngroups: int,
                     pos_fw: torch.Tensor, neg_fw: torch.Tensor, pos_bw: torch.Tensor, neg_bw: torch.Tensor,
                     colsum_ws: torch.Tensor, *, eps: float = 1e-9, scale_fw: float = 1.0, scale_bw: float = 1.0) -> None:
    """Outputs may be fp32, bf16 or split fp16 and wider than (S / nq): padding columns are zero-filled.  scale_fw /
    scale_bw multiply the forward / backward tables (powers of two that keep a split-fp16 table's lo halves in the
    fp16 normal range; the consumer undoes them in its alpha)."""
    _need_cuda(z, enc_len, group_meta, pos_fw, neg_fw, pos_bw, neg_bw, colsum_ws)
    B, nq, S = z.shape
    # algorithmic bytes: z read once, the four normalised weight tables written once (incl. their zero K padding)
    osz = pos_fw.element_size()
    with _timed("stcexp_normalize", 6.0 * B * nq * S,
                B * nq * S * 4.0 + 2.0 * B * nq * pos_fw.shape[-1] * osz + 2.0 * B * S * pos_bw.shape[-1] * osz):
        _hip.check(_hip.load().odic_stcexp_normalize(_p(z), _p(enc_len), _p(group_meta), ngroups, _p(pos_fw),
                                                     _p(neg_fw), pos_fw.shape[-1], _p(pos_bw), _p(neg_bw),
                                                     pos_bw.shape[-1], _p(colsum_ws), B, nq, S, eps, scale_fw, scale_bw,
                                                     dtype_code(pos_fw.dtype), _stream()), "odic_stcexp_normalize")


def selector_mix(x, ldx, sel_pre, lds, a, lda, b, ldb, out, ldo, M, d) -> None:
    _need_cuda(x, sel_pre, a, b, out)
    with _timed("selector_mix", 6.0 * M * d, 5.0 * M * d * 4):     # x, selector, A', B' in; y out
        _hip.check(_hip.load().odic_selector_mix(_p(x), ldx, _p(sel_pre), lds, _p(a), lda, _p(b), ldb, _p(out), ldo,
                                                 M, d, _stream()), "odic_selector_mix")


# ----------------------------------------------------------------------------------------------
def dec_embed(tokens, embed, pos_table, pos, y, ldy, N, d, scale) -> None:
    _need_cuda(tokens, embed, pos_table, pos, y)
    with _timed("dec_embed", 2.0 * N * d, N * (8.0 + 2 * d * 4) + d * 4):     # token id, embedding row in, y row out, one pos row
        _hip.check(_hip.load().odic_dec_embed(_p(tokens), _p(embed), _p(pos_table), _p(pos), _p(y), ldy, N, d,
                                              pos_table.shape[0], scale, _stream()), "odic_dec_embed")


def dynexp_step(lin, ldlin, qexp, bexp, cond_c, key_c, va_c, vb_c, wfa_c, wfb_c, qk_c, anc, row_valid, pos,
                y_in, ldy_in, y, ldy, N, T, d, E, eps=1e-9) -> None:
    _need_cuda(lin, qexp, bexp, cond_c, key_c, va_c, vb_c, wfa_c, wfb_c, qk_c, anc, row_valid, pos, y_in, y)
    # algorithmic bytes of one incremental step at position t (layers.py:152-204 on the newest row only, in the
    # re-associated form of csrc/decoder_ops.hip): in  lin [N,5d], y_in; through the ancestor table, per earlier
    # position cond, key, va, vb [d each], its (j+1)·E forward weights (x2) and query·key [E];  out  the position's
    # cache rows and y.   t = the host's step hint, else the mean position of a T-long search.
    t = _STEP_T if _STEP_T is not None else (T - 1) / 2.0
    nbytes = N * ((5 * d + 2 * d) * 4.0 + (t + 1) * (4 * d + E) * 4.0 + (t + 1) * (t + 2) * E * 4.0
                  + (4 * d + 2 * (t + 1) * E + E) * 4.0 + (t + 1) * 4.0)
    flops = N * ((2 * t + E + 1) * 2.0 * d + 6.0 * (t + 1) * d + 2.0 * (t + 1) * (t + 2) * E)
    with _timed("dynexp_step", flops, nbytes):
        _hip.check(_hip.load().odic_dynexp_step(_p(lin), ldlin, _p(qexp), _p(bexp), _p(cond_c), _p(key_c), _p(va_c),
                                                _p(vb_c), _p(wfa_c), _p(wfb_c), _p(qk_c), _p(anc), _p(row_valid),
                                                _p(pos), _p(y_in), ldy_in, _p(y), ldy, N, T, d, E, eps,
                                                _stream()),
                   "odic_dynexp_step")


# ----------------------------------------------------------------------------------------------
# whole-sequence (teacher-forced) decoder pass — csrc/decoder_seq.hip
def dec_embed_seq(tokens, embed, pos_table, y, ldy, N, T, d, scale, dec_len=None, row_valid=None) -> None:
    """y[n·T + t] = embed[tokens[n, t]]·scale + pos_table[t]; with dec_len / row_valid also the [N·T] row mask."""
    _need_cuda(tokens, embed, pos_table, y, dec_len, row_valid)
    with _timed("dec_embed", 2.0 * N * T * d, N * T * (8.0 + 2 * d * 4) + T * d * 4):
        _hip.check(_hip.load().odic_dec_embed_seq(_p(tokens), _p(embed), _p(pos_table), _p(dec_len), _p(row_valid),
                                                  _p(y), ldy, N, T, d, embed.shape[0], pos_table.shape[0], scale,
                                                  _stream()), "odic_dec_embed_seq")


def dynexp_seq(lin, ldlin, qexp, bexp, dec_len, y_in, ldy_in, y, ldy, N, T, d, E, eps=1e-9) -> None:
    """Dynamic expansion of all T positions of N sequences (layers.py:152-204) in one launch."""
    _need_cuda(lin, qexp, bexp, dec_len, y_in, y)
    # lin rows in, y in / out;  (T+E)·T dot products of length d, the T³E/6 coefficient sums (5 flops each, x2),
    # 4 FMAs per (t, i <= t, channel)
    flops = N * (2.0 * (T + E) * T * d + 10.0 * T * T * T * E / 6 + 4.0 * T * T * d)
    with _timed("dynexp_seq", flops, N * T * (5 * d + 2 * d) * 4.0):
        _hip.check(_hip.load().odic_dynexp_seq(_p(lin), ldlin, _p(qexp), _p(bexp), _p(dec_len), _p(y_in), ldy_in,
                                               _p(y), ldy, N, T, d, E, eps, _stream()), "odic_dynexp_seq")


def dynexp_fill_caches(lin, ldlin, qexp, cache: dict, n_seq, P, rows_per_image, N_cache, T_cache, d, E, eps=1e-9) -> None:
    """The step caches `cache` (one layer's dict of a DecodeState: cond, key, va, vb, wfa, wfb, qk) for positions 0..P-1 of
    n_seq sequences, slot i·rows_per_image, from the lin rows of the whole-sequence pass (odic_dynexp_fill_caches)."""
    c = cache
    _need_cuda(lin, qexp, *(c[k] for k in ("cond", "key", "va", "vb", "wfa", "wfb", "qk")))
    # lin rows in; the four row caches, qk and the P(P+1)/2·E forward weights (x2) out;  (P+E)·P dot products of length d
    with _timed("dynexp_fill", n_seq * 2.0 * (P + E) * P * d, n_seq * (P * 9.0 * d + P * E + P * (P + 1.0) * E) * 4.0):
        _hip.check(_hip.load().odic_dynexp_fill_caches(_p(lin), ldlin, _p(qexp), _p(c["cond"]), _p(c["key"]), _p(c["va"]),
                                                       _p(c["vb"]), _p(c["wfa"]), _p(c["wfb"]), _p(c["qk"]), n_seq, P,
                                                       rows_per_image, N_cache, T_cache, d, E, eps, _stream()),
                   "odic_dynexp_fill_caches")


def token_stats(logits, ldl, target, logp_target, sum_logp, argmax, max_logp, status, R, V) -> None:
    """Per logits row: log-prob of the target, Σ_v log-prob, arg-max (ties → lower index) and its log-prob."""
    _need_cuda(logits, target, logp_target, sum_logp, argmax, max_logp, status)
    with _timed("token_stats", 4.0 * R * V, R * V * 4.0 + R * 24.0):
        _hip.check(_hip.load().odic_token_stats(_p(logits), ldl, _p(target), _p(logp_target), _p(sum_logp), _p(argmax),
                                                _p(max_logp), _p(status), R, V, _stream()), "odic_token_stats")


def cross_attn_step(q, ldq, kv, ldkv, koff, voff, enc_len, row_valid, out, ldo, N, n_img, S, d, heads) -> None:
    _need_cuda(q, kv, enc_len, row_valid, out)
    # q and out rows per sequence, K and V of the S encoder tokens ONCE per image (shared by its beams)
    with _timed("cross_attn_step", 4.0 * N * S * d, (2.0 * N * d + 2.0 * n_img * S * d) * 4):
        _hip.check(_hip.load().odic_cross_attn_step(_p(q), ldq, _p(kv), ldkv, koff, voff, _p(enc_len), _p(row_valid),
                                                    _p(out), ldo, N, n_img, S, d, heads, _stream()),
                   "odic_cross_attn_step")


def cross_attn_probs(q, ldq, kv, ldkv, koff, enc_len, row_valid, out, ldo, N, n_img, S, d, heads, per_head=False,
                     accumulate=False, scale=1.0) -> None:
    """The cross-attention probabilities of N query rows (odic_cross_attn_step's q, kv, enc_len, row_valid):
    out [N, S] = scale·Σ_h p_h, or with per_head out [N, heads·S] = scale·p_h at column h·S + s; accumulate adds to out."""
    _need_cuda(q, kv, enc_len, row_valid, out)
    with _timed("cross_attn_probs", 2.0 * N * S * d, (N * d + n_img * S * d + N * S * (heads if per_head else 1)) * 4.0):
        _hip.check(_hip.load().odic_cross_attn_probs(_p(q), ldq, _p(kv), ldkv, koff, _p(enc_len), _p(row_valid), _p(out),
                                                     ldo, N, n_img, S, d, heads, int(bool(per_head)),
                                                     int(bool(accumulate)), scale, _stream()),
                   "odic_cross_attn_probs")


def logsoftmax_topk(logits, ldl, logp_out, ldp, top_val, top_idx, N, V, k) -> None:
    _need_cuda(logits, logp_out, top_val, top_idx)
    with _timed("logsoftmax_topk", 4.0 * N * V, N * V * 4.0 * (2 if logp_out is not None else 1) + N * k * 8.0):
        _hip.check(_hip.load().odic_logsoftmax_topk(_p(logits), ldl, _p(logp_out), ldp, _p(top_val), _p(top_idx), N, V,
                                                    k, _stream()), "odic_logsoftmax_topk")


def logsoftmax_sample(logits, ldl, logp_out, ldp, top_val, top_idx, N, V, k, seed: int, pos=None) -> None:
    """k words per row drawn without replacement from softmax(logits) on the device (Gumbel-top-k, Philox noise
    keyed by `seed`, the row, the word and *pos) + their log-probs — the reference's multinomial draws."""
    _need_cuda(logits, logp_out, top_val, top_idx, pos)
    with _timed("logsoftmax_topk", 14.0 * N * V, N * V * 4.0 * (2 if logp_out is not None else 1) + N * k * 8.0):
        _hip.check(_hip.load().odic_logsoftmax_sample(_p(logits), ldl, _p(logp_out), ldp, _p(top_val), _p(top_idx), N, V,
                                                      k, seed & 0xFFFFFFFFFFFFFFFF, _p(pos), _stream()),
                   "odic_logsoftmax_sample")


def logsoftmax_sample_scored(logits, ldl, logp_out, ldp, top_val, top_idx, top_pert, N, V, k, seed: int, pos=None) -> None:
    """logsoftmax_sample that also writes the perturbed scores of its draws, top_pert fp32 [N, k] = log-prob + Gumbel noise
    (odic_logsoftmax_sample_scored): what stochastic_beam_step ranks captions by.  Words and log-probs are those of
    logsoftmax_sample for the same seed and *pos, bit for bit."""
    _need_cuda(logits, logp_out, top_val, top_idx, top_pert, pos)
    with _timed("logsoftmax_topk", 14.0 * N * V, N * V * 4.0 * (2 if logp_out is not None else 1) + N * k * 12.0):
        _hip.check(_hip.load().odic_logsoftmax_sample_scored(_p(logits), ldl, _p(logp_out), ldp, _p(top_val), _p(top_idx),
                                                             _p(top_pert), N, V, k, seed & 0xFFFFFFFFFFFFFFFF, _p(pos),
                                                             _stream()), "odic_logsoftmax_sample_scored")


def sample_filter(temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> "_hip.SampleFilter":
    """odic_sample_filter of the three controls; 1/temperature is formed in double and rounded once to fp32."""
    return _hip.SampleFilter(1.0 / float(temperature), int(top_k), float(top_p))


def logsoftmax_sample_filtered(logits, ldl, logp_out, ldp, top_val, top_idx, kept, N, V, k, flt, seed: int, pos=None) -> None:
    """logsoftmax_sample's draws from the temperature-scaled top-k / nucleus set of `flt` (sample_filter(...)); top_val and
    logp_out stay the model's own log-probs.  kept: int32 [N] for the size of every row's filtered set, or None."""
    _need_cuda(logits, logp_out, top_val, top_idx, kept, pos)
    # the plain draw's work plus the passes of the threshold search over the row: 32 bisection rounds per active control
    rounds = 32 * ((0 < flt.top_k < V) + (flt.top_p < 1.0))
    with _timed("logsoftmax_sample_filtered", (14.0 + 3.0 * rounds) * N * V,
                N * V * 4.0 * (2 if logp_out is not None else 1) + N * k * 8.0):
        _hip.check(_hip.load().odic_logsoftmax_sample_filtered(_p(logits), ldl, _p(logp_out), ldp, _p(top_val), _p(top_idx),
                                                               _p(kept), N, V, k, C.byref(flt),
                                                               seed & 0xFFFFFFFFFFFFFFFF, _p(pos), _stream()),
                   "odic_logsoftmax_sample_filtered")


def cider_workspace(R: int, device) -> torch.Tensor:
    """int64 [R, CIDER_ROW_WORDS]: one odic_cider_vectorize row per caption (cider_row_views names its parts)."""
    return torch.empty(R, _hip.CIDER_ROW_WORDS, dtype=torch.int64, device=device)


def cider_row_views(ws: torch.Tensor):
    """→ (keys int64 [R, 512] — the uint64 bits, weights fp64 [R, 512], norms fp64 [R, 4], meta int32 [R, 2] = count, length)."""
    nk = _hip.CIDER_MAX_KEYS
    return (ws[:, :nk], ws[:, nk:2 * nk].view(torch.float64), ws[:, 2 * nk:2 * nk + 4].view(torch.float64),
            ws[:, 2 * nk + 4:2 * nk + 5].view(torch.int32))


def cider_vectorize(tokens: torch.Tensor, lengths: torch.Tensor, ws: torch.Tensor, *, max_id: int = _hip.CIDER_MAX_ID,
                    df_keys=None, df_idf=None, default_idf: float = 1.0) -> None:
    """Captions (int32 tokens [R, ld], lengths [R]) → their TF-IDF n-gram rows in `ws` (odic_cider_vectorize).  df_keys: the
    sorted uint64 keys of the document-frequency table as int64 bits, df_idf their fp64 IDF; without a table every n-gram
    weighs default_idf."""
    _need_cuda(tokens, lengths, ws, df_keys, df_idf)
    if tokens.dtype != torch.int32 or lengths.dtype != torch.int32 or ws.dtype != torch.int64:
        raise ValueError("cider_vectorize takes int32 tokens and lengths and an int64 workspace")
    if tokens.dim() != 2 or tokens.stride(1) != 1 or ws.dim() != 2 or ws.stride(1) != 1 or not lengths.is_contiguous():
        raise ValueError("cider_vectorize takes row-major operands")
    R, T = tokens.shape
    if T > _hip.CIDER_MAX_LEN:
        raise ValueError(f"captions of {T} tokens exceed the limit of {_hip.CIDER_MAX_LEN}")
    if not 0 <= max_id <= _hip.CIDER_MAX_ID:
        raise ValueError(f"word ids up to {max_id} exceed the n-gram key's limit of {_hip.CIDER_MAX_ID}")
    if lengths.numel() != R or ws.shape[0] < R or ws.shape[1] < _hip.CIDER_ROW_WORDS:
        raise ValueError("cider_vectorize: lengths or workspace do not cover the captions")
    n_table = 0 if df_keys is None else df_keys.numel()
    with _timed("cider_vectorize", 0.0, R * (T * 4.0 + 16.0 * _hip.CIDER_MAX_KEYS)):
        _hip.check(_hip.load().odic_cider_vectorize(_p(tokens), tokens.stride(0), _p(lengths), R, T, max_id, _p(df_keys),
                                                    _p(df_idf), n_table, float(default_idf), _p(ws), ws.stride(0),
                                                    _stream()), "odic_cider_vectorize")


def cider_pairs(ws: torch.Tensor, ref_begin: torch.Tensor, ref_end: torch.Tensor, sim: torch.Tensor) -> None:
    """sim fp64 [H, max_refs]: CIDEr-D of hypothesis h (row h of `ws`) against each of the rows [ref_begin[h], ref_end[h]);
    unused slots are written as 0 (odic_cider_pairs)."""
    _need_cuda(ws, ref_begin, ref_end, sim)
    if ref_begin.dtype != torch.int32 or ref_end.dtype != torch.int32 or sim.dtype != torch.float64:
        raise ValueError("cider_pairs takes int32 row ranges and an fp64 output")
    H, max_refs = sim.shape
    if ref_begin.numel() != H or ref_end.numel() != H or sim.stride(1) != 1:
        raise ValueError("cider_pairs: one row range per hypothesis, a row-major output")
    with _timed("cider_pairs", 0.0, 16.0 * _hip.CIDER_MAX_KEYS * H * (1 + max_refs)):
        _hip.check(_hip.load().odic_cider_pairs(_p(ws), ws.stride(0), ws.shape[0], _p(ref_begin), _p(ref_end), H, max_refs,
                                                _p(sim), sim.stride(0), _stream()), "odic_cider_pairs")


def bleu_stats(ws: torch.Tensor, lengths: torch.Tensor, max_len: int, hyp_row: torch.Tensor, ref_begin: torch.Tensor,
               ref_end: torch.Tensor, stats: torch.Tensor) -> None:
    """stats int32 [Q, >= 12]: the BLEU components of query q = (hypothesis row hyp_row[q], reference rows [ref_begin[q],
    ref_end[q])) of the workspace `ws` (odic_bleu_stats).  `ws` must hold the rows cider_vectorize writes WITHOUT a table
    and with default_idf = 1.0; `lengths` and `max_len` are the ones it was given."""
    _need_cuda(ws, lengths, hyp_row, ref_begin, ref_end, stats)
    if any(t.dtype != torch.int32 for t in (lengths, hyp_row, ref_begin, ref_end, stats)) or ws.dtype != torch.int64:
        raise ValueError("bleu_stats takes an int64 workspace and int32 lengths, queries and output")
    if ws.dim() != 2 or ws.stride(1) != 1 or stats.dim() != 2 or stats.stride(1) != 1 or not lengths.is_contiguous():
        raise ValueError("bleu_stats takes row-major operands")
    R, Q = ws.shape[0], stats.shape[0]
    if lengths.numel() != R or ws.shape[1] < _hip.CIDER_ROW_WORDS or stats.shape[1] < _hip.BLEU_STAT_WORDS:
        raise ValueError("bleu_stats: lengths, workspace or output rows are too short")
    if any(t.numel() != Q or not t.is_contiguous() for t in (hyp_row, ref_begin, ref_end)):
        raise ValueError("bleu_stats: one hypothesis row and one row range per query")
    with _timed("bleu_stats", 0.0, 16.0 * _hip.CIDER_MAX_KEYS * 2 * Q):
        _hip.check(_hip.load().odic_bleu_stats(_p(ws), ws.stride(0), _p(lengths), R, int(max_len), _p(hyp_row),
                                               _p(ref_begin), _p(ref_end), Q, _p(stats), stats.stride(0), _stream()),
                   "odic_bleu_stats")


def lcs_pairs(tokens: torch.Tensor, lengths: torch.Tensor, ref_begin: torch.Tensor, ref_end: torch.Tensor,
              lcs: torch.Tensor) -> None:
    """lcs int32 [H, max_refs]: the longest-common-subsequence length of caption h (row h of int32 tokens [R, ld], lengths
    [R]) with each of the rows [ref_begin[h], ref_end[h]); unused slots are written as 0 (odic_lcs_pairs)."""
    _need_cuda(tokens, lengths, ref_begin, ref_end, lcs)
    if any(t.dtype != torch.int32 for t in (tokens, lengths, ref_begin, ref_end, lcs)):
        raise ValueError("lcs_pairs takes int32 operands")
    if tokens.dim() != 2 or tokens.stride(1) != 1 or lcs.dim() != 2 or lcs.stride(1) != 1 or not lengths.is_contiguous():
        raise ValueError("lcs_pairs takes row-major operands")
    R, T = tokens.shape
    H, max_refs = lcs.shape
    if T > _hip.CIDER_MAX_LEN:
        raise ValueError(f"captions of {T} tokens exceed the limit of {_hip.CIDER_MAX_LEN}")
    if lengths.numel() != R or any(t.numel() != H or not t.is_contiguous() for t in (ref_begin, ref_end)):
        raise ValueError("lcs_pairs: one length per caption, one row range per hypothesis")
    with _timed("lcs_pairs", 0.0, 8.0 * T * H * max_refs):
        _hip.check(_hip.load().odic_lcs_pairs(_p(tokens), tokens.stride(0), _p(lengths), R, T, _p(ref_begin), _p(ref_end), H,
                                              max_refs, _p(lcs), lcs.stride(0), _stream()), "odic_lcs_pairs")


def ensemble_logprobs(logits_list, out: torch.Tensor) -> None:
    """out[n] = log(mean_m softmax(logits_m[n])) — ensemble_captioning_model.py:66-83."""
    _need_cuda(out, *logits_list)
    M = len(logits_list)
    N, V = out.shape
    arr = (C.c_void_p * M)(*[t.data_ptr() for t in logits_list])
    with _timed("ensemble_logprobs", 0.0, 4.0 * (M + 1) * N * V):
        _hip.check(_hip.load().odic_ensemble_logprobs(arr, M, logits_list[0].stride(0), _p(out), out.stride(0), N, V,
                                                      _stream()), "odic_ensemble_logprobs")


def topk_rows(logp: torch.Tensor, top_val: torch.Tensor, top_idx: torch.Tensor, k: int) -> None:
    _need_cuda(logp, top_val, top_idx)
    N, V = logp.shape
    with _timed("logsoftmax_topk", 0.0, 4.0 * N * V):
        _hip.check(_hip.load().odic_topk_rows(_p(logp), logp.stride(0), _p(top_val), _p(top_idx), N, V, k, _stream()),
                   "odic_topk_rows")


def search_constraints(tokens: torch.Tensor, pos: torch.Tensor, T: int, eos_idx: int, *, row_valid=None, banned=None,
                       no_repeat_ngram: int = 0, min_words: int = 0) -> "_hip.SearchConstraints":
    """odic_search_constraints for topk_rows_constrained (the caller keeps the tensors alive).  tokens: int64 prefixes,
    N·T elements (the beam state's `tokens`); pos: the device int32 step counter; row_valid: int32 [N] or None;
    banned: int32 device tensor of word ids or None."""
    _need_cuda(tokens, pos, row_valid, banned)
    if tokens.dtype != torch.int64 or pos.dtype != torch.int32 or not tokens.is_contiguous():
        raise ValueError("search_constraints: tokens must be contiguous int64 and pos int32")
    for name, t in (("row_valid", row_valid), ("banned", banned)):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()):
            raise ValueError(f"search_constraints: {name} must be a contiguous int32 tensor")
    n_banned = 0 if banned is None else banned.numel()
    return _hip.SearchConstraints(_p(tokens), _p(pos), _p(row_valid), _p(banned) if n_banned else None, n_banned,
                                  int(no_repeat_ngram), int(min_words), int(eos_idx), int(T))


def topk_rows_constrained(logp: torch.Tensor, constraints: "_hip.SearchConstraints", top_val: torch.Tensor,
                          top_idx: torch.Tensor, k: int) -> None:
    """The k best admissible words of every row of logp [N, V] (log-probs, taken as they are) under `constraints`
    (odic_topk_rows_constrained): banned words, EOS before the minimum length, words that would repeat an n-gram."""
    _need_cuda(logp, top_val, top_idx)
    N, V = logp.shape
    with _timed("logsoftmax_topk", 0.0, 4.0 * N * V):
        _hip.check(_hip.load().odic_topk_rows_constrained(_p(logp), logp.stride(0), C.byref(constraints), _p(top_val),
                                                          _p(top_idx), N, V, k, _stream()),
                   "odic_topk_rows_constrained")


def contrast_args(weight: float, plausibility: float, floor: float, min_keep: int) -> "_hip.ContrastArgs":
    """odic_contrast_args: the suppressor's weight, log(plausibility) rounded once to fp32 (-inf for 0 = no cut), the
    suppressor floor and the least number of candidates the cut leaves."""
    log_alpha = math.log(plausibility) if plausibility > 0.0 else float("-inf")
    return _hip.ContrastArgs(float(weight), log_alpha, float(floor), int(min_keep))


def contrast_topk(logits_list, count: Optional[torch.Tensor], args: "_hip.ContrastArgs", top_val: torch.Tensor,
                  top_idx: torch.Tensor, k: int, *, score_out: Optional[torch.Tensor] = None,
                  kept: Optional[torch.Tensor] = None) -> None:
    """The k best contrastive scores of every row (odic_contrast_topk): logits_list[0] the target's logits [N, V], the
    others the distractors' (one row pitch); count int32 [N]: how many of them row n uses (None with the target alone).
    score_out [N, V]: the whole score row, for topk_rows_constrained; kept int32 [N]: the plausible words per row."""
    _need_cuda(count, top_val, top_idx, score_out, kept, *logits_list)
    M = len(logits_list)
    N, V = logits_list[0].shape
    ldl = logits_list[0].stride(0)
    if any(t.shape != (N, V) or t.stride(0) != ldl or t.stride(1) != 1 or t.dtype != torch.float32 for t in logits_list):
        raise ValueError("contrast_topk: the logits must be fp32 [N, V] tensors of one shape and row pitch")
    if count is not None and (count.dtype != torch.int32 or count.numel() != N or not count.is_contiguous()):
        raise ValueError("contrast_topk: count must be a contiguous int32 [N] tensor")
    arr = (C.c_void_p * M)(*[t.data_ptr() for t in logits_list])
    with _timed("contrast_topk", (4.0 + 6.0 * (M - 1)) * N * V,
                4.0 * N * V * (M + (1 if score_out is not None else 0)) + N * k * 8.0):
        _hip.check(_hip.load().odic_contrast_topk(arr, M, ldl, _p(count), C.byref(args), _p(score_out),
                                                  score_out.stride(0) if score_out is not None else 0, _p(top_val),
                                                  _p(top_idx), _p(kept), N, V, k, _stream()), "odic_contrast_topk")


def embed_args(embed, pos_table, y, ldy, d, scale) -> "_hip.EmbedArgs":
    """odic_embed_args for beam_step / beam_reset (the caller keeps the tensors alive)."""
    _need_cuda(embed, pos_table, y)
    return _hip.EmbedArgs(_p(embed), _p(pos_table), _p(y), ldy, d, scale, pos_table.shape[0])


def _emb_ref(emb):
    return C.byref(emb) if emb is not None else None


def _beam_bytes(n_img, beams, T, emb):
    # the k prefixes (token int64, log-prob, ancestor) of t+1 positions read and re-written, per-beam flags, and
    # with the embedding tail one table row in and one input row out per beam
    t = _STEP_T if _STEP_T is not None else (T - 1) / 2.0
    return n_img * (2.0 * beams * (t + 1) * 16.0 + beams * 32.0 + (beams * emb.d * 8.0 if emb is not None else 0.0))


def beam_step(cand_val, cand_idx, state: "_hip.BeamState", n_img, beams, T, eos_idx, emb=None) -> None:
    with _timed("beam_step", 0.0, n_img * beams * beams * 8.0 + _beam_bytes(n_img, beams, T, emb)):
        _hip.check(_hip.load().odic_beam_step(_p(cand_val), _p(cand_idx), C.byref(state), _emb_ref(emb), n_img, beams,
                                              T, eos_idx, _stream()), "odic_beam_step")


def group_beam_step(cand_val, cand_idx, state: "_hip.BeamState", n_img, groups, group_beams, T, eos_idx, penalty,
                    emb=None) -> None:
    """The step of diverse beam search (odic_group_beam_step): `groups` groups of `group_beams` beams per image choose
    in turn, each paying `penalty` per earlier group that took the same word.  cand_* are [n_img·R, R], R = groups·group_beams."""
    beams = groups * group_beams
    with _timed("beam_step", 0.0, n_img * beams * beams * 8.0 + _beam_bytes(n_img, beams, T, emb)):
        _hip.check(_hip.load().odic_group_beam_step(_p(cand_val), _p(cand_idx), beams, C.byref(state), _emb_ref(emb), n_img,
                                                    groups, group_beams, T, eos_idx, penalty, _stream()),
                   "odic_group_beam_step")


def require_beam_step(cand_val, cand_idx, logp, required, state: "_hip.BeamState", n_img, bank_beams, T, eos_idx,
                      emb=None) -> None:
    """The step of a search for captions that contain given words (odic_require_beam_step).  required: int64 [n_img, C]
    on the device (-1 = unused slot) or None for C = 0; the image's R = 2^C·bank_beams rows are 2^C banks of bank_beams
    beams.  cand_* are [n_img·R, R]; logp fp32 [n_img·R, V] (row stride >= V): the log-prob rows the candidates came from."""
    C_ = 0 if required is None else int(required.shape[1])
    if C_:
        _need_cuda(logp, required)
        if required.dtype != torch.int64 or required.dim() != 2 or required.shape[0] != n_img or not required.is_contiguous():
            raise ValueError("require_beam_step: required must be a contiguous int64 [n_img, C] tensor")
        if logp.dtype != torch.float32 or logp.dim() != 2 or logp.stride(1) != 1:
            raise ValueError("require_beam_step: logp must be fp32 [N, V] with unit column stride")
    beams = bank_beams << C_ if 0 <= C_ <= 4 else 0
    V = int(logp.shape[1]) if logp is not None else int(eos_idx) + 1
    ldl = int(logp.stride(0)) if logp is not None else V
    with _timed("beam_step", 0.0, n_img * beams * (beams * 8.0 + C_ * 12.0) + _beam_bytes(n_img, beams, T, emb)):
        _hip.check(_hip.load().odic_require_beam_step(_p(cand_val), _p(cand_idx), beams, _p(logp), ldl, _p(required) if C_ else None, C_, C.byref(state), _emb_ref(emb),
                                                      n_img, bank_beams, T, eos_idx, V, _stream()),
                   "odic_require_beam_step")


def stochastic_beam_step(cand_val, cand_idx, cand_pert, gscore, state: "_hip.BeamState", n_img, beams, T, eos_idx,
                         emb=None) -> None:
    """The step of stochastic beam search (odic_stochastic_beam_step; Kool et al. 2019): the `beams` rows of an image
    become its `beams` continuations with the largest perturbed scores — captions sampled without replacement.  cand_*
    are [n_img·beams, beams] as logsoftmax_sample_scored writes them with k = beams; gscore fp32 [n_img·beams] carries the
    rows' perturbed scores from step to step (read from *pos = 1 on, written at every step)."""
    _need_cuda(cand_val, cand_idx, cand_pert, gscore)
    with _timed("beam_step", 0.0, n_img * beams * (beams * 12.0 + 8.0) + _beam_bytes(n_img, beams, T, emb)):
        _hip.check(_hip.load().odic_stochastic_beam_step(_p(cand_val), _p(cand_idx), _p(cand_pert), _p(gscore),
                                                         C.byref(state), _emb_ref(emb), n_img, beams, T, eos_idx,
                                                         _stream()), "odic_stochastic_beam_step")


def pool_scale(T: int, length_penalty: float) -> torch.Tensor:
    """scale[L] = float32(float64(L) ** length_penalty), L = 0 .. T: the table odic_pool_beam_step divides a hypothesis's sum
    by (host tensor; the power in float64, then one rounding — the device never calls powf)."""
    return torch.tensor([float(L) ** float(length_penalty) for L in range(T + 1)], dtype=torch.float64).to(torch.float32)


class Pool:
    """The pool of finished hypotheses of a pooled beam search (odic_pool_args) for n_img images, P = beams slots each and
    T positions, with its tensors: tokens, logprobs [n_img, P, T]; len, sum, score, serial [n_img, P]; count, closed
    [n_img]; scale [T + 1]."""

    def __init__(self, n_img: int, beams: int, T: int, length_penalty: float, min_words: int, early_stopping: bool, device):
        z = lambda dt, *s: torch.zeros(*s, dtype=dt, device=device)      # noqa: E731
        self.tokens, self.logprobs = z(torch.int64, n_img, beams, T), z(torch.float32, n_img, beams, T)
        self.len, self.serial = z(torch.int32, n_img, beams), z(torch.int32, n_img, beams)
        self.sum, self.score = z(torch.float32, n_img, beams), z(torch.float32, n_img, beams)
        self.count, self.closed = z(torch.int32, n_img), z(torch.int32, n_img)
        self.scale = pool_scale(T, length_penalty).to(device)
        self.args = pool_args(self.tokens, self.logprobs, self.len, self.sum, self.score, self.serial, self.count,
                              self.closed, self.scale, min_words, early_stopping)


def pool_args(tokens, logprobs, len_, sum_, score, serial, count, closed, scale, min_words: int,
              early_stopping: bool) -> "_hip.PoolArgs":
    """odic_pool_args (the caller keeps the tensors alive)."""
    _need_cuda(tokens, logprobs, len_, sum_, score, serial, count, closed, scale)
    for name, t, dt in (("tokens", tokens, torch.int64), ("logprobs", logprobs, torch.float32), ("len", len_, torch.int32),
                        ("sum", sum_, torch.float32), ("score", score, torch.float32), ("serial", serial, torch.int32),
                        ("count", count, torch.int32), ("closed", closed, torch.int32), ("scale", scale, torch.float32)):
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"pool_args: {name} must be a contiguous {dt} tensor")
    return _hip.PoolArgs(*(_p(t) for t in (tokens, logprobs, len_, sum_, score, serial, count, closed, scale)),
                         int(min_words), 1 if early_stopping else 0)


def pool_reset(pool: "_hip.PoolArgs", n_img: int) -> None:
    """An empty pool and every image open (odic_pool_reset: count = closed = 0)."""
    with _timed("beam_reset", 0.0, n_img * 8.0):
        _hip.check(_hip.load().odic_pool_reset(C.byref(pool), n_img, _stream()), "odic_pool_reset")


def pool_beam_step(cand_val, cand_idx, logp, pool: "_hip.PoolArgs", state: "_hip.BeamState", n_img, beams, T, eos_idx,
                   emb=None) -> None:
    """The step of pooled beam search (odic_pool_beam_step): cand_* [n_img·beams, beams] hold every row's best words other
    than EOS, logp fp32 [n_img·beams, V] the log-prob rows they came from (EOS's log-prob is read there); a hypothesis
    that takes EOS goes to the pool, the rows stay live, an image whose pool cannot be improved closes."""
    _need_cuda(cand_val, cand_idx, logp)
    if logp.dtype != torch.float32 or logp.dim() != 2 or logp.stride(1) != 1:
        raise ValueError("pool_beam_step: logp must be fp32 [N, V] with unit column stride")
    with _timed("beam_step", 0.0, n_img * beams * (beams * 8.0 + 4.0 + 2 * T * 12.0) + _beam_bytes(n_img, beams, T, emb)):
        _hip.check(_hip.load().odic_pool_beam_step(_p(cand_val), _p(cand_idx), _p(logp), int(logp.stride(0)), C.byref(pool),
                                                   C.byref(state), _emb_ref(emb), n_img, beams, T, eos_idx,
                                                   int(logp.shape[1]), _stream()), "odic_pool_beam_step")


def pool_beam_finalize(pool: "_hip.PoolArgs", state: "_hip.BeamState", order, score, n_img, beams, T) -> None:
    """odic_pool_beam_finalize: the rows an open image still grows join its pool; order int32 / score fp32 [n_img, beams]:
    the pool's slots best first (-1 / -inf behind the image's count)."""
    _need_cuda(order, score)
    with _timed("beam_finalize", 0.0, n_img * beams * (32.0 + 2 * T * 12.0)):
        _hip.check(_hip.load().odic_pool_beam_finalize(C.byref(pool), C.byref(state), _p(order), _p(score), n_img, beams, T,
                                                       _stream()), "odic_pool_beam_finalize")


def beam_finalize(state: "_hip.BeamState", order, score, n_img, beams) -> None:
    with _timed("beam_finalize", 0.0, n_img * beams * 16.0):
        _hip.check(_hip.load().odic_beam_finalize(C.byref(state), _p(order), _p(score), n_img, beams, _stream()),
                   "odic_beam_finalize")


def beam_finalize_best(state: "_hip.BeamState", order, score, out_tok, out_len, n_img, beams, T, pad_idx) -> None:
    """Final ranking + the best caption per image as an int32 [n_img, T] row padded with `pad_idx` and its length."""
    _need_cuda(order, score, out_tok, out_len)
    with _timed("beam_finalize", 0.0, n_img * (beams * 8.0 + T * 12.0)):
        _hip.check(_hip.load().odic_beam_finalize_best(C.byref(state), _p(order), _p(score), _p(out_tok), _p(out_len),
                                                       n_img, beams, T, pad_idx, _stream()), "odic_beam_finalize_best")


def beam_reset(state: "_hip.BeamState", n_img, beams, T, sos_idx, emb=None) -> None:
    with _timed("beam_reset", 0.0, n_img * beams * (28.0 + (emb.d * 4.0 if emb is not None else 0.0))):
        _hip.check(_hip.load().odic_beam_reset(C.byref(state), _emb_ref(emb), n_img, beams, T, sos_idx, _stream()),
                   "odic_beam_reset")


def beam_reset_prefix(state: "_hip.BeamState", prefix, prefix_logp, n_img, beams, group_beams, T, sos_idx, emb=None) -> None:
    """The beam state behind a prefix (odic_beam_reset_prefix): prefix int64 [n_img, P], prefix_logp fp32 [n_img, P]."""
    _need_cuda(prefix, prefix_logp)
    if prefix.dtype != torch.int64 or prefix_logp.dtype != torch.float32 or prefix.dim() != 2 or \
            tuple(prefix.shape) != tuple(prefix_logp.shape) or prefix.shape[0] != n_img or \
            not prefix.is_contiguous() or not prefix_logp.is_contiguous():
        raise ValueError("beam_reset_prefix: prefix int64 and prefix_logp fp32, both contiguous [n_img, P]")
    P = prefix.shape[1]
    with _timed("beam_reset", 0.0, n_img * (P * 12.0 + beams * ((P + 1) * 16.0 + 28.0 + (emb.d * 4.0 if emb is not None else 0.0)))):
        _hip.check(_hip.load().odic_beam_reset_prefix(C.byref(state), _emb_ref(emb), _p(prefix), _p(prefix_logp), n_img,
                                                      beams, group_beams, T, P, sos_idx, _stream()),
                   "odic_beam_reset_prefix")


def quantize_fp8_per_channel(w: torch.Tensor):
    """Weight-pack-time plumbing of the fp8 mode: W fp32 [N, K] → (fp8 e4m3 [N, K], scale fp32 [N]) with
    W ≈ fp8·scale[:, None], scale = max|row| / 448 (the whole e4m3 range per output channel)."""
    w = w.detach().float()
    scale = (w.abs().amax(dim=1).clamp_min(1e-12) / FP8_MAX)
    q = (w / scale[:, None]).clamp(-FP8_MAX, FP8_MAX).cpu().to(FP8_DTYPE)        # host cast: exact OCP round-to-nearest-even
    return q.to(w.device).contiguous(), scale.contiguous()
