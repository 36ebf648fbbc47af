"""Host-side sequencing of the HIP kernels: Swin backbone, expansion encoder, incremental decoder.

Everything here is plumbing: weights are packed once per (state dict, device, precision) into the
layouts the kernels want, activations live in torch-owned device buffers, and every arithmetic
step is a call into libodic_hip.so on the current stream (so a whole forward can be captured into
a hipGraph by `torch.cuda.graph`).  There is no CPU path.

Data layout in HBM
  * residual stream            fp32 [B·L, C]  (both precisions; 24 blocks deep, kept exact)
  * LN outputs / qkv / attention out / MLP hidden   fp32 or bf16 [B·L, *] token-major, never
    window-permuted: the (shifted) window gather/scatter happens inside the attention kernel
  * encoder / decoder          fp32; per-layer residual streams are column slices of one
    [rows, N_layers·d] buffer so the reference's torch.cat (End_ExpansionNet_v2.py:97,133) is free
  * decoder caches             [T, N, ...] indexed by (position, slot) + an ancestor table
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass, fields
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _hip, ops
from .search import check_constraints
from .weights import Geometry

SD = Dict[str, torch.Tensor]
# precision → dtype of the backbone's bf16-class activations / weights.  "fp8" (BASELINE.json configs[4]) keeps that
# at bf16 for the patch-merge reductions and the backbone output, and runs the Swin blocks with fp8 GEMM operands
# (qkv, fc1, fc2: 11/12 of the block FLOPs) and fp16 qkv / attention activations (proj on the fp16 MFMA).
# "x3" (the near-exact fast mode): activations and weights travel as split-fp16 pairs (ops.H2_DTYPE: hi + lo, 22
# significand bits, 4 bytes per element) and every contraction of the backbone and of the expansion encoder is three
# fp16 MFMAs (csrc/gemm_x3.hip, window_attention_h2_kernel); residual streams, normalisations and the decoder are fp32.
_CDT = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": torch.bfloat16, "x3": ops.H2_DTYPE}


def pack_operand(t: torch.Tensor, cdt) -> Tuple[torch.Tensor, float]:
    """fp32 weight [N, K] → (GEMM operand in the engine's dtype, alpha that undoes its pack-time scale).  Split-fp16
    operands are scaled by a power of two so that the lo halves are fp16 normals (exact to undo)."""
    if cdt == ops.H2_DTYPE:
        sc = ops.pow2_scale_for_h2(t)
        return ops.h2_from_f32(t * sc), 1.0 / sc
    return t.to(cdt).contiguous(), 1.0


def _dev(t: torch.Tensor, device, dtype=None) -> torch.Tensor:
    t = t.detach()
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to(device).contiguous()


# =================================================================================================
# Swin backbone  
# =================================================================================================
@dataclass
class SwinFlags:
    """The backbone's environment switches, parsed once per engine: what each selects and what it measured is DESIGN.md §5.
    The fusions are bf16-only; a switch that does not apply to the engine's precision is off."""
    ln_read: bool                       # ODIC_FUSE_BACKBONE_LN_READ: width 192, norm → qkv and norm → fc1 as one launch each
    fuse_qkv_attn: bool                 # ODIC_FUSE_QKV_ATTENTION: width 192, norm1 → qkv → attention core as one launch
    fuse_qkv_attn_tiled: bool           # ODIC_FUSE_QKV_ATTENTION_TILED: the wider stages, qkv → attention core as one launch
    fuse_qkv_attn_tiled_min_c: int      # ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C: the narrowest width that takes it (384 adds stage 1)
    fuse_mlp: bool                      # ODIC_FUSE_MLP: width 192, norm2 → fc1 → GELU → fc2 + residual as one launch
    stage_chunks: List[int]             # ODIC_SWIN_CHUNKS: image chunks a stage's blocks run over, per stage

    @classmethod
    def from_env(cls, precision: str) -> "SwinFlags":
        env = os.environ
        on = lambda name: precision == "bf16" and env.get(name, "1") == "1"        # noqa: E731
        lr = env.get("ODIC_FUSE_BACKBONE_LN_READ", "1")                            # split fp16: opt-in, =x3
        return cls(ln_read=(precision == "bf16" and lr != "0") or (precision == "x3" and lr == "x3"),
                   fuse_qkv_attn=on("ODIC_FUSE_QKV_ATTENTION"), fuse_qkv_attn_tiled=on("ODIC_FUSE_QKV_ATTENTION_TILED"),
                   fuse_qkv_attn_tiled_min_c=int(env.get("ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C", "768")),
                   fuse_mlp=on("ODIC_FUSE_MLP"), stage_chunks=[int(v) for v in env.get("ODIC_SWIN_CHUNKS", "1").split(",")])


# The forms of a block's attention half (what runs in front of proj) and of its MLP half; their launches: DESIGN.md §5.
ATTN_FP8, ATTN_FUSED, ATTN_LN_READ, ATTN_TILED, ATTN_PLAIN = "fp8", "fused", "ln_read", "tiled", "plain"
MLP_FP8, MLP_FUSED, MLP_LN_READ, MLP_PLAIN = "fp8", "fused", "ln_read", "plain"


def swin_block_plan(precision: str, flags: SwinFlags, C_: int, heads: int, ws: int, res: int, M: int, *, dense: bool,
                    folded: bool, qkv_a_one: bool, calibrating: bool, fp8_ready: bool) -> Tuple[str, str]:
    """(attention form, MLP form) of one Swin block over M rows: `dense` — it has the packed bias of the fast attention
    kernels, `folded` — it has the `*_lnr` weights, `qkv_a_one` — its qkv operand carries no pack-time scale, `calibrating` —
    the pass records operand ranges (`_amax`) and so needs the LayerNorm outputs and the hidden activations in memory."""
    cdt = _CDT[precision]
    if fp8_ready and not calibrating:
        return ATTN_FP8, MLP_FP8
    # The folded weights serve BOTH halves, and both hang on the predicate of the qkv product's shape (M x 3C x C) — the
    # MLP forms too, whose own product is M x 4C x C.  Kept as it has always been.
    if folded and not calibrating and ops.a_ln_supported(M, 3 * C_, C_, cdt):
        return (ATTN_FUSED if flags.fuse_qkv_attn and ws == 12 and dense else ATTN_LN_READ,
                MLP_FUSED if flags.fuse_mlp and ops.swin_mlp_supported(M, C_, cdt) else MLP_LN_READ)
    tiled = (flags.fuse_qkv_attn_tiled and not calibrating and dense and qkv_a_one and C_ >= flags.fuse_qkv_attn_tiled_min_c
             and ops.swin_qkv_attention_tiled_supported(M, C_, heads, ws, res, cdt))
    return ATTN_TILED if tiled else ATTN_PLAIN, MLP_PLAIN


class SwinEngine:
    def __init__(self, sd: SD, g: Geometry, device, precision: str = "fp32", calibration_images=None):
        if precision not in _CDT:
            raise ValueError(f"precision must be one of {list(_CDT)}")
        self.g, self.device, self.precision = g, device, precision
        self.cdt = _CDT[precision]
        self.flags = SwinFlags.from_env(precision)
        fast_attn = precision in ("bf16", "fp8", "x3")
        P = "swin_transf"
        f32 = lambda k: _dev(sd[k], device, torch.float32)          # noqa: E731
        cw = lambda k: pack_operand(_dev(sd[k], device, torch.float32), self.cdt)      # noqa: E731  (operand, alpha)
        self.pe_w = _dev(sd[f"{P}.patch_embed.proj.weight"].reshape(g.swin_embed_dim, -1), device, torch.float32)
        self.pe_b = f32(f"{P}.patch_embed.proj.bias")
        self.pe_g, self.pe_beta = f32(f"{P}.patch_embed.norm.weight"), f32(f"{P}.patch_embed.norm.bias")
        self.stages = []
        for s, depth in enumerate(g.swin_depths):
            blocks = []
            for b in range(depth):
                p = f"{P}.layers.{s}.blocks.{b}"
                (qkv_w, qkv_a), (proj_w, proj_a) = cw(p + ".attn.qkv.weight"), cw(p + ".attn.proj.weight")
                (fc1_w, fc1_a), (fc2_w, fc2_a) = cw(p + ".mlp.fc1.weight"), cw(p + ".mlp.fc2.weight")
                table = f32(p + ".attn.relative_position_bias_table")
                w = dict(
                    n1w=f32(p + ".norm1.weight"), n1b=f32(p + ".norm1.bias"),
                    qkv_w=qkv_w, qkv_a=qkv_a, qkv_b=f32(p + ".attn.qkv.bias"), table=table,
                    dense=(ops.shifted_bias_prescaled(table, g.stage_window(s), (g.stage_dim(s) // g.swin_num_heads[s]) ** -0.5)
                           if fast_attn and g.stage_window(s) == 12 else None),
                    proj_w=proj_w, proj_a=proj_a, proj_b=f32(p + ".attn.proj.bias"),
                    n2w=f32(p + ".norm2.weight"), n2b=f32(p + ".norm2.bias"),
                    fc1_w=fc1_w, fc1_a=fc1_a, fc1_b=f32(p + ".mlp.fc1.bias"),
                    fc2_w=fc2_w, fc2_a=fc2_a, fc2_b=f32(p + ".mlp.fc2.bias"),
                    shift=g.stage_shift(s, b))
                if self.flags.ln_read and g.stage_dim(s) == 192:
                    # LayerNorm-while-reading: gamma / beta folded into the fp32 weight, which is then packed like every other
                    for name, lin, norm in (("qkv", ".attn.qkv", "n1"), ("fc1", ".mlp.fc1", "n2")):
                        Wg, b2, _ = ops.fold_layernorm(f32(p + lin + ".weight"), w[name + "_b"], w[norm + "w"], w[norm + "b"])
                        op, alpha = pack_operand(Wg, self.cdt)
                        w[name + "_lnr"] = (op, b2, alpha)
                blocks.append(w)
            down = None
            if s < len(g.swin_depths) - 1:
                p = f"{P}.layers.{s}.downsample"
                red_w, red_a = cw(p + ".reduction.weight")
                down = dict(nw=f32(p + ".norm.weight"), nb=f32(p + ".norm.bias"), red_w=red_w, red_a=red_a)
            self.stages.append((blocks, down))
        self.fn_w, self.fn_b = f32(f"{P}.norm.weight"), f32(f"{P}.norm.bias")
        self.fp8_ready = False
        if precision == "fp8":
            self._pack_fp8(sd, calibration_images)

    # ------------------------------------------------------------------------------------------ fp8 mode
    def _pack_fp8(self, sd: SD, calibration_images) -> None:
        """Static quantisation of the Swin blocks: per-output-channel fp8 weights for qkv / fc1 / fc2, fp16 weights
        for proj, and per-tensor activation scales (LayerNorm outputs, GELU hidden) calibrated on one bf16 pass over
        `calibration_images` (default: two synthetic images) — amax x 1.25 mapped to the e4m3 maximum.  The activation
        scale of a LayerNorm output is folded into its gamma / beta, the product (activation scale x weight channel
        scale) is the consuming GEMM's `col_scale`, the GELU hidden is written as fp8 through `out_scale`."""
        from .weights import synth_images
        g, dv = self.g, self.device
        if any(g.stage_window(s) != 12 or g.stage_dim(s) % 64 for s in range(len(g.swin_depths))):
            raise RuntimeError("fp8 mode needs 12x12 windows and stage widths that are multiples of 64 (Swin-L: 192·2^s)")
        img = calibration_images if calibration_images is not None else synth_images(2, g, seed=7)
        amax = {}
        self.forward(img.to(dv, torch.float32), _amax=amax)                 # bf16 pass recording the operand ranges
        P = "swin_transf"
        margin = 1.25
        self.fp8_range = {k: margin * v for k, v in amax.items()}           # what each static scale can represent
        for s, (blocks, _) in enumerate(self.stages):
            for b, w in enumerate(blocks):
                p = f"{P}.layers.{s}.blocks.{b}"
                s1 = margin * amax[(s, b, "ln1")] / ops.FP8_MAX
                s2 = margin * amax[(s, b, "ln2")] / ops.FP8_MAX
                sh = margin * amax[(s, b, "hid")] / ops.FP8_MAX
                f32 = lambda k: _dev(sd[k], dv, torch.float32)      # noqa: E731
                q_qkv, sw_qkv = ops.quantize_fp8_per_channel(f32(p + ".attn.qkv.weight"))
                q_fc1, sw_fc1 = ops.quantize_fp8_per_channel(f32(p + ".mlp.fc1.weight"))
                q_fc2, sw_fc2 = ops.quantize_fp8_per_channel(f32(p + ".mlp.fc2.weight"))
                w.update(dict(
                    n1w8=(w["n1w"] / s1).contiguous(), n1b8=(w["n1b"] / s1).contiguous(),
                    n2w8=(w["n2w"] / s2).contiguous(), n2b8=(w["n2b"] / s2).contiguous(),
                    qkv_w8=q_qkv, qkv_cs=(sw_qkv * s1).contiguous(),
                    fc1_w8=q_fc1, fc1_cs=(sw_fc1 * s2).contiguous(), hid_inv=1.0 / sh,
                    fc2_w8=q_fc2, fc2_cs=(sw_fc2 * sh).contiguous(),
                    proj_w16=f32(p + ".attn.proj.weight").to(torch.float16).contiguous()))
        self.fp8_ready = True

    def fp8_saturation(self, img: torch.Tensor) -> dict:
        """Observed operand ranges of `img` (one bf16 pass) against the calibrated fp8 ranges: the tensors whose
        amax exceeds what the static scale represents are cast with clipping at ±448."""
        if not self.fp8_ready:
            raise RuntimeError("not an fp8 engine")
        seen = {}
        self.forward(img, _amax=seen)
        ratios = {k: seen[k] / self.fp8_range[k] for k in seen}
        over = {f"s{k[0]}b{k[1]}.{k[2]}": round(v, 3) for k, v in ratios.items() if v > 1.0}
        return {"tensors": len(ratios), "clipping_tensors": len(over), "worst_ratio": round(max(ratios.values()), 3),
                "median_ratio": round(sorted(ratios.values())[len(ratios) // 2], 3), "clipping": over}

    def forward(self, img: torch.Tensor, taps: Optional[dict] = None, out_dtype=torch.float32,
                _amax: Optional[dict] = None) -> torch.Tensor:
        """img fp32 [B,3,H,W] on the engine's device → features [B, res_last², C_last] (`out_dtype`)."""
        g, cdt = self.g, self.cdt
        if img.dtype != torch.float32 or not img.is_cuda:
            raise RuntimeError("SwinEngine.forward wants an fp32 CUDA image batch")
        img = img.contiguous()
        B = img.shape[0]
        x = ops.patch_embed(img, self.pe_w, self.pe_b, self.pe_g, self.pe_beta, g.swin_patch_size)
        if taps is not None:
            taps["patch_embed"] = x.clone()
        for s, (blocks, down) in enumerate(self.stages):
            res, C_, heads, ws = g.stage_res(s), g.stage_dim(s), g.swin_num_heads[s], g.stage_window(s)
            x = x.view(B * res * res, C_)
            # image chunks (stage_chunks): a stage's blocks run over B/n images at a time, so that what one launch
            # writes (qkv, the MLP hidden, the residual stream) is still in the 256 MB Infinity Cache when the
            # next launch reads it — the stage-0/1 launches are HBM-bound
            n_ch = self.stage_chunks[s] if s < len(self.stage_chunks) else 1
            if taps is not None or _amax is not None or n_ch < 1 or B % n_ch:
                n_ch = 1
            x_all, B_all = x, B
            B = B_all // n_ch
            for ci, bi, w in ((ci, bi, w) for ci in range(n_ch) for bi, w in enumerate(blocks)):
                x = x_all[ci * B * res * res:(ci + 1) * B * res * res]
                attn, mlp = swin_block_plan(self.precision, self.flags, C_, heads, ws, res, x.shape[0],
                                            dense=w["dense"] is not None, folded="qkv_lnr" in w, qkv_a_one=w["qkv_a"] == 1.0,
                                            calibrating=_amax is not None, fp8_ready=self.fp8_ready)
                # ---- attention half: x → att
                if attn == ATTN_FP8:            # LN → fp8 | qkv: fp8 MFMA → fp16 | attention fp16 | proj: fp16 MFMA + residual
                    xn = ops.layernorm(x, w["n1w8"], w["n1b8"], out_dtype=ops.FP8_DTYPE)
                    qkv = ops.gemm(xn, w["qkv_w8"], w["qkv_b"], col_scale=w["qkv_cs"], out_dtype=torch.float16)
                elif attn == ATTN_FUSED:        # q / k / v never leave the chip
                    att = ops.swin_qkv_attention(x, w["qkv_lnr"][0], w["qkv_lnr"][1], w["dense"], B, res, C_, heads, ws, w["shift"])
                elif attn == ATTN_LN_READ:
                    qkv = ops.gemm(None, w["qkv_lnr"][0], w["qkv_lnr"][1], a_ln=x, out_dtype=cdt, alpha=w["qkv_lnr"][2])
                else:
                    xn = ops.layernorm(x, w["n1w"], w["n1b"], out_dtype=cdt)
                    if _amax is not None:
                        _amax[(s, bi, "ln1")] = float(xn.float().abs().max())
                    if attn == ATTN_TILED:      # q / k / v never leave the chip
                        att = ops.swin_qkv_attention_tiled(xn, w["qkv_w"], w["qkv_b"], w["dense"], B, res, C_, heads, ws, w["shift"])
                    else:
                        qkv = ops.gemm(xn, w["qkv_w"], w["qkv_b"], alpha=w["qkv_a"])
                if attn not in (ATTN_FUSED, ATTN_TILED):
                    att = ops.window_attention(qkv, w["table"], B, res, C_, heads, ws, w["shift"], bias_shifted_prescaled=w["dense"])
                # ---- proj + residual (fp8 mode: the fp16 weight; its proj_a is 1)
                ops.gemm(att, w["proj_w16" if attn == ATTN_FP8 else "proj_w"], w["proj_b"], residual=x, out=x, alpha=w["proj_a"])
                # ---- MLP half: x += fc2(GELU(fc1(LN(x))))
                if mlp == MLP_FP8:              # LN → fp8 | fc1: fp8 MFMA + GELU → fp8 | fc2: fp8 MFMA + residual
                    xn = ops.layernorm(x, w["n2w8"], w["n2b8"], out_dtype=ops.FP8_DTYPE)
                    h = ops.gemm(xn, w["fc1_w8"], w["fc1_b"], act=ops.ACT_GELU, col_scale=w["fc1_cs"], out_scale=w["hid_inv"],
                                 out_dtype=ops.FP8_DTYPE)
                elif mlp == MLP_FUSED:          # the hidden activations never leave the chip
                    ops.swin_mlp(x, w["fc1_lnr"][0], w["fc1_lnr"][1], w["fc2_w"], w["fc2_b"], w["fc2_a"], out=x)
                elif mlp == MLP_LN_READ:
                    h = ops.gemm(None, w["fc1_lnr"][0], w["fc1_lnr"][1], a_ln=x, act=ops.ACT_GELU, out_dtype=cdt, alpha=w["fc1_lnr"][2])
                else:
                    xn = ops.layernorm(x, w["n2w"], w["n2b"], out_dtype=cdt)
                    h = ops.gemm(xn, w["fc1_w"], w["fc1_b"], act=ops.ACT_GELU, alpha=w["fc1_a"])
                    if _amax is not None:
                        _amax[(s, bi, "ln2")] = float(xn.float().abs().max())
                        _amax[(s, bi, "hid")] = float(h.float().abs().max())
                if mlp != MLP_FUSED:            # (fp8 mode: the fp8 weight with its column scales; its fc2_a is 1)
                    fc2_w, fc2_cs = (w["fc2_w8"], w["fc2_cs"]) if mlp == MLP_FP8 else (w["fc2_w"], None)
                    ops.gemm(h, fc2_w, w["fc2_b"], residual=x, out=x, alpha=w["fc2_a"], col_scale=fc2_cs)
                if taps is not None:
                    taps[f"s{s}b{bi}"] = x.view(B, res * res, C_).clone()
            x, B = x_all, B_all
            if down is not None:
                xm = ops.patch_merge_layernorm(x, down["nw"], down["nb"], B, res, C_, out_dtype=cdt)
                x = ops.gemm(xm.view(-1, 4 * C_), down["red_w"], out_dtype=torch.float32, alpha=down["red_a"])
                if taps is not None:
                    taps[f"merge{s}"] = x.view(B, (res // 2) ** 2, 2 * C_).clone()
        res = g.stage_res(len(g.swin_depths) - 1)
        out = ops.layernorm(x, self.fn_w, self.fn_b, out_dtype=out_dtype)
        return out.view(B, res * res, -1)


for _f in fields(SwinFlags):       # eng.fuse_mlp, eng.stage_chunks, ... read and write eng.flags (a test flips them on a live engine)
    setattr(SwinEngine, _f.name, property(lambda self, _n=_f.name: getattr(self.flags, _n),
                                          lambda self, v, _n=_f.name: setattr(self.flags, _n, v)))


# =================================================================================================
# Expansion encoder + decoder, fp32
# =================================================================================================
class DecodeState:
    """Device-resident state of one search / teacher-forced run (see include/odic_hip.h)."""

    def __init__(self, eng: "CaptionerEngine", n_img: int, beams: int, T: int, kv: torch.Tensor,
                 enc_len: torch.Tensor, S: int):
        g, dv = eng.g, eng.device
        N = n_img * beams
        d, E, L = g.d_model, g.num_exp_dec, g.N_dec
        self.n_img, self.beams, self.N, self.T, self.S = n_img, beams, N, T, S
        self.kv, self.enc_len = kv, enc_len
        f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dv)      # noqa: E731
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dv)      # noqa: E731
        self.ycat = f(N, L * d)
        # what step_logits would otherwise build again for every token: each layer's (input, output) column slices of
        # ycat (layer 0 works in place), and the integers ops.gemm_dims derives at each of its call sites — the operand
        # shapes and strides of a site are the same at every step of this state
        self.layer_io = [(self.ycat[:, max(i - 1, 0) * d:max(i, 1) * d], self.ycat[:, i * d:(i + 1) * d]) for i in range(L)]
        self.gemm_dims: dict = {}
        self.caches = [dict(cond=f(T, N, d), key=f(T, N, d), va=f(T, N, d), vb=f(T, N, d),
                            wfa=f(T, N, T, E), wfb=f(T, N, T, E), qk=f(T, N, E)) for _ in range(L)]
        self.anc = i32(N, T)
        self.row_valid = torch.ones(N, dtype=torch.int32, device=dv)
        self.next_tok = torch.zeros(N, dtype=torch.int64, device=dv)
        self.pos, self.done, self.ctr = i32(1), i32(1), i32(1)
        self.tokens = torch.zeros(n_img, beams, T, dtype=torch.int64, device=dv)
        self.logprobs = f(n_img, beams, T)
        self.cumul, self.n_elem, self.has_eos = f(N), i32(N), i32(N)
        self.cand_val, self.cand_idx = f(N, beams), i32(N, beams)
        self.logits = f(N, g.vocab_size)
        self.logp = None            # [N, V] log-probs, allocated by the first constrained step (odic_topk_rows_constrained)
        self.cand_pert = None       # [N, beams] perturbed scores of the candidates, and
        self.gscore = None          # [N] of the rows: allocated by the first stochastic beam step
        self.banned = None          # int32 word ids of the constraints built for this state (kept alive here)
        self.beam_state = _hip.BeamState(*(t.data_ptr() for t in (
            self.tokens, self.logprobs, self.anc, self.cumul, self.n_elem, self.has_eos, self.row_valid,
            self.next_tok, self.pos, self.done, self.ctr)))
        # the next position's input embedding, written by the launch that chooses the words (odic_embed_args)
        self.emb = ops.embed_args(eng.embed, eng.pos_table, self.ycat, L * d, d, math.sqrt(d))


class CaptionerEngine:
    """precision 'fp32': everything exact fp32.  'bf16': the ENCODER's products run on the bf16 MFMA
    GEMM (fp32 accumulation, fp32 residual streams, fp32 normalisations); the decoder stays fp32."""

    def __init__(self, sd: SD, g: Geometry, device, precision: str = "fp32"):
        self.g, self.device, self.precision = g, device, precision
        self.cdt = _CDT[precision]
        # decoder LayerNorms folded into the consuming skinny GEMM (10 fewer launches per step; see
        # odic_gemm_args.ln_colsum).  ODIC_FOLD_LN=0 keeps the separate odic_layernorm launches.
        self.fuse_ln = os.environ.get("ODIC_FOLD_LN", "1") == "1"
        self._pad_ws = {}           # encode's zero-padded GEMM outputs, kept per (B, S, stream)
        d = g.d_model
        f32 = lambda k: _dev(sd[k], device, torch.float32)          # noqa: E731
        cat = lambda ks: torch.cat([f32(k) for k in ks], 0).contiguous()   # noqa: E731
        cw = lambda t: pack_operand(t, self.cdt)                    # noqa: E731  (encoder GEMM operand, alpha)
        (self.in_w, self.in_a), self.in_b = cw(f32("input_linear.weight")), f32("input_linear.bias")
        self.enc = []
        for i in range(g.N_enc):
            p = f"encoders.{i}"
            s = p + ".stc_exp"
            q, q_a = cw(f32(s + ".query_exp_vectors.weight"))
            key_w, key_a = cw(f32(s + ".key_embed.weight"))
            sel_w, sel_a = cw(f32(s + ".selector_embed.weight"))
            ab_w, ab_a = cw(cat([s + ".class_a_embed.weight", s + ".class_b_embed.weight"]))  # [2d, d]
            f1w, f1a = cw(f32(p + ".ff.linear_1.weight"))
            f2w, f2a = cw(f32(p + ".ff.linear_2.weight"))
            self.enc.append(dict(
                n1w=f32(p + ".norm_1.weight"), n1b=f32(p + ".norm_1.bias"),
                n2w=f32(p + ".norm_2.weight"), n2b=f32(p + ".norm_2.bias"),
                q=q, q_a=q_a,
                bvT=f32(s + ".bias_exp_vectors.weight").t().contiguous(),              # [d, nq] fp32
                key_w=key_w, key_a=key_a, key_b=f32(s + ".key_embed.bias"),
                sel_w=sel_w, sel_a=sel_a, sel_b=f32(s + ".selector_embed.bias"),
                ab_w=ab_w, ab_a=ab_a,
                ab_b=cat([s + ".class_a_embed.bias", s + ".class_b_embed.bias"]),
                f1w=f1w, f1a=f1a, f1b=f32(p + ".ff.linear_1.bias"),
                f2w=f2w, f2a=f2a, f2b=f32(p + ".ff.linear_2.bias")))
        (self.er_w, self.er_a), self.er_b = cw(f32("enc_reduce_group.weight")), f32("enc_reduce_group.bias")
        self.ern_w, self.ern_b = f32("enc_reduce_norm.weight"), f32("enc_reduce_norm.bias")
        self.group_meta = ops.stcexp_group_meta(g.num_exp_enc_list, device)
        self.dec = []
        kvw, kvb = [], []
        for i in range(g.N_dec):
            p = f"decoders.{i}"
            s = p + ".dyn_exp"
            names = ["cond_embed", "key_linear", "class_a_embed", "class_b_embed", "selector_embed"]
            self.dec.append(dict(
                n1w=f32(p + ".norm_1.weight"), n1b=f32(p + ".norm_1.bias"),
                n2w=f32(p + ".norm_2.weight"), n2b=f32(p + ".norm_2.bias"),
                n3w=f32(p + ".norm_3.weight"), n3b=f32(p + ".norm_3.bias"),
                dyn_w=cat([f"{s}.{n}.weight" for n in names]), dyn_b=cat([f"{s}.{n}.bias" for n in names]),
                qexp=f32(s + ".query_exp_vectors.weight"), bexp=f32(s + ".bias_exp_vectors.weight"),
                wq=f32(p + ".mha.Wq.weight"), bq=f32(p + ".mha.Wq.bias"),
                wo=f32(p + ".mha.out_linear.weight"), bo=f32(p + ".mha.out_linear.bias"),
                f1w=f32(p + ".ff.linear_1.weight"), f1b=f32(p + ".ff.linear_1.bias"),
                f2w=f32(p + ".ff.linear_2.weight"), f2b=f32(p + ".ff.linear_2.bias")))
            w = self.dec[-1]
            w["dyn_f"] = ops.fold_layernorm(w["dyn_w"], w["dyn_b"], w["n1w"], w["n1b"])
            w["wq_f"] = ops.fold_layernorm(w["wq"], w["bq"], w["n2w"], w["n2b"])
            w["f1_f"] = ops.fold_layernorm(w["f1w"], w["f1b"], w["n3w"], w["n3b"])
            kvw += [p + ".mha.Wk.weight", p + ".mha.Wv.weight"]
            kvb += [p + ".mha.Wk.bias", p + ".mha.Wv.bias"]
        self.kv_w32, self.kv_b = cat(kvw), cat(kvb)                 # [2·N_dec·d, d]
        self.kv_w, self.kv_a = cw(self.kv_w32)
        self.dr_w, self.dr_b = f32("dec_reduce_group.weight"), f32("dec_reduce_group.bias")
        self.drn_w, self.drn_b = f32("dec_reduce_norm.weight"), f32("dec_reduce_norm.bias")
        self.voc_w, self.voc_b = f32("vocab_linear.weight"), f32("vocab_linear.bias")
        self.voc_f = ops.fold_layernorm(self.voc_w, self.voc_b, self.drn_w, self.drn_b)
        self.embed, self.pos_table = f32("out_embedder.embed.weight"), f32("pos_encoder.weight")

    # ------------------------------------------------------------------------------------------
    def _as_operand(self, x: torch.Tensor) -> torch.Tensor:
        """fp32 activations → the encoder GEMM operand dtype (identity view in fp32 mode)."""
        if x.dtype == self.cdt:
            return x
        if self.cdt == torch.bfloat16 and x.dtype == torch.float32:
            return ops.cast_bf16(x)
        if self.cdt == ops.H2_DTYPE and x.dtype == torch.float32:
            return ops.cast_h2(x)
        raise RuntimeError(f"cannot feed {x.dtype} to a {self.cdt} encoder")

    def encode(self, feats: torch.Tensor, enc_len: torch.Tensor, want_bf16_mem: bool = False):
        """feats [B,S,F] (fp32, or bf16 in bf16 mode) → encoder output fp32 [B,S,d]  (forward_enc after
        the backbone: End_ExpansionNet_v2.py:82-101 / ExpansionNet_v2.py:52-70).  enc_len int32 [B]."""
        g, dv, cdt = self.g, self.device, self.cdt
        B, S, F = feats.shape
        d, L, nq, M = g.d_model, g.N_enc, sum(g.num_exp_enc_list), B * S
        x3 = cdt == ops.H2_DTYPE
        pad = 64 if cdt == torch.bfloat16 else (32 if x3 else 1)   # the bf16 / split-fp16 GEMMs need K % 64 / 32 == 0
        # split fp16: the normalised expansion weights (<= 1, typically 1e-2 forward / 1e-3 backward) are written
        # scaled by a power of two so that their lo halves stay fp16 normals; undone in the consuming product's alpha
        fw_sc, bw_sc = (256.0, 4096.0) if x3 else (1.0, 1.0)
        Sp, nqp = -(-S // pad) * pad, -(-nq // pad) * pad
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dv)      # noqa: E731
        zc = lambda *s: torch.zeros(*s, dtype=cdt, device=dv)               # noqa: E731  (K padding must be finite)
        x0 = ops.gemm(self._as_operand(feats.contiguous().view(M, F)), self.in_w, self.in_b, out_dtype=torch.float32,
                      alpha=self.in_a)                                                                   # [M,d]
        xcat = f(M, L * d)
        z = f(B, nq, S)
        # K-padded operands.  odic_stcexp_normalize writes its four outputs out to their leading dimension (zeros in the
        # padding), so they need no clearing; the three GEMM outputs whose padding columns no launch ever writes are kept
        # per (shape, stream) and zeroed ONCE — clearing them inside every captured encode pass was seven fill launches
        # (both halves of this contract are pinned by tests/test_containment_gpu.py: odic_gemm leaves columns [N, ldc) untouched
        # for every tile configuration — test_gemm_engine_padded_products_verbatim — and the result of a call does not depend
        # on the call before it — test_encode_is_independent_of_the_previous_call)
        ec = lambda *s: torch.empty(*s, dtype=cdt, device=dv)               # noqa: E731
        pf, nf = ec(B, nq, Sp), ec(B, nq, Sp)
        pb, nb = ec(B, S, nqp), ec(B, S, nqp)
        colsum = f(B * len(g.num_exp_enc_list) * 2 * S)
        key = (B, S, torch.cuda.current_stream(dv).cuda_stream)
        pads = self._pad_ws.get(key)
        if pads is None:
            pads = (zc(B, d, nqp), zc(B, d, nqp), zc(B, 2 * d, Sp))
            if not torch.cuda.is_current_stream_capturing():  # (a first call under capture: plain per-call buffers)
                self._pad_ws[key] = pads
        AT, BT, vabT = pads
        A2, B2 = f(B, S, d), f(B, S, d)
        key = torch.empty(M, d, dtype=cdt, device=dv)
        for i, w in enumerate(self.enc):
            xin = x0 if i == 0 else xcat[:, (i - 1) * d:i * d]
            xo = xcat[:, i * d:(i + 1) * d]
            x2 = ops.layernorm(xin, w["n1w"], w["n1b"], out_dtype=cdt)
            ops.gemm(x2, w["key_w"], w["key_b"], out=key, alpha=w["key_a"])
            sel = ops.gemm(x2, w["sel_w"], w["sel_b"], out_dtype=torch.float32, alpha=w["sel_a"])
            # (class_a | class_b) projections, produced transposed: [B, 2d, S] = W·x2ᵀ + b(row)
            ops.gemm(w["ab_w"], x2.view(B, S, d), w["ab_b"], out=vabT, bias_axis=1, batch=B, alpha=w["ab_a"])
            # z = Q·Kᵀ/sqrt(d)
            ops.gemm(w["q"], key.view(B, S, d), out=z, batch=B, alpha=w["q_a"] / math.sqrt(d))
            ops.stcexp_normalize(z, enc_len, self.group_meta, len(g.num_exp_enc_list), pf, nf, pb, nb, colsum,
                                 scale_fw=fw_sc, scale_bw=bw_sc)
            # class_aᵀ [d,nq] = Vaᵀ·pos_fwᵀ + Bvᵀ    (layers.py:63-64, transposed)
            ops.gemm(vabT[:, :d], pf, residual=w["bvT"], out=AT, batch=B, alpha=1.0 / fw_sc)
            ops.gemm(vabT[:, d:], nf, residual=w["bvT"], out=BT, batch=B, alpha=1.0 / fw_sc)
            # backward: [S,nq]·[nq,d]
            ops.gemm(pb, AT, out=A2, batch=B, alpha=1.0 / bw_sc)
            ops.gemm(nb, BT, out=B2, batch=B, alpha=1.0 / bw_sc)
            ops.selector_mix(xin, xin.stride(0), sel, d, A2, d, B2, d, xo, xo.stride(0), M, d)
            x2 = ops.layernorm(xo, w["n2w"], w["n2b"], out_dtype=cdt)
            h = ops.gemm(x2, w["f1w"], w["f1b"], act=ops.ACT_RELU, alpha=w["f1a"])
            ops.gemm(h, w["f2w"], w["f2b"], residual=xo, out=xo, alpha=w["f2a"])
        pre = ops.gemm(self._as_operand(xcat), self.er_w, self.er_b, residual=xcat[:, (L - 1) * d:], out=f(M, d),
                       alpha=self.er_a)
        mem = ops.layernorm(pre, self.ern_w, self.ern_b).view(B, S, d)
        if want_bf16_mem and cdt != torch.float32:                 # the K/V projection's operand, rounded once
            return mem, ops.layernorm(pre, self.ern_w, self.ern_b, out_dtype=cdt).view(B, S, d)
        return mem

    def project_kv(self, mem: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Cross-attention K/V of every decoder layer, once per image (the reference recomputes them
        every step for every beam, layers.py:274-276): [B,S,d] → [B,S,2·N_dec·d]."""
        B, S, d = mem.shape
        n = self.kv_w.shape[0]
        if out is None:
            out = torch.empty(B, S, n, dtype=torch.float32, device=self.device)
        # bf16 mode: the product runs on the bf16 MFMA GEMM whatever dtype the caller holds the memory in, so
        # the direct beam_search call and CaptionPipeline (which feeds the bf16 LayerNorm output) see
        # bit-identical K/V: round-to-nearest-even of the same fp32 values either way.
        ops.gemm(self._as_operand(mem.contiguous().view(B * S, d)), self.kv_w, self.kv_b, out=out, alpha=self.kv_a)
        return out

    # ------------------------------------------------------------------------------------------
    def new_state(self, n_img: int, beams: int, T: int, kv: torch.Tensor, enc_len: torch.Tensor) -> DecodeState:
        if T > 128:
            raise RuntimeError("decode length > 128 positions is not supported by odic_dynexp_step")
        if T - 1 > self.pos_table.shape[0]:
            raise RuntimeError(f"{T - 1} decode positions exceed the pos_encoder table ({self.pos_table.shape[0]})")
        return DecodeState(self, n_img, beams, T, kv, enc_len, kv.shape[1])

    def step_logits(self, st: DecodeState, embed: bool = True) -> None:
        """Process position *st.pos for every sequence: next_tok → st.logits [N,V].  embed=False: the input row of
        this position is already in st.ycat (written by the launch that chose the word: beam_reset / beam_step
        with st.emb)."""
        g = self.g
        d, N = g.d_model, st.N
        if embed:
            ops.dec_embed(st.next_tok, self.embed, self.pos_table, st.pos, st.ycat, st.ycat.stride(0), N, d, math.sqrt(d))
        # the folded-LayerNorm form lives in the skinny-M kernel (M <= 192 rows, gemm_f32.hip); wider
        # searches (batch 64 x beam 5, decode groups) take the LayerNorm + GEMM pair
        fuse = self.fuse_ln and N <= 192
        eps = 1e-5

        dims = st.gemm_dims.setdefault(fuse, {})

        def gemm(site, A, W, b, residual=None, out=None, **kw):
            """ops.gemm with the integers of this call site derived once per state (DecodeState.gemm_dims)."""
            dm = dims.get(site)
            if dm is None:
                dm = dims[site] = ops.gemm_dims(A, W, residual, out)
            return ops.gemm(A, W, b, residual, out, dims=dm, **kw)

        def ln_gemm(site, x, nw, nb, W, b, folded, **kw):
            """LayerNorm(x)·Wᵀ + b: one launch (LayerNorm folded into the product) or two."""
            if fuse:
                Wf, bf, cs = folded
                return gemm(site, x, Wf, bf, ln_fold=(cs, eps), **kw)
            return gemm(site, ops.layernorm(x, nw, nb), W, b, **kw)

        for i, w in enumerate(self.dec):
            c = st.caches[i]
            xin, xo = st.layer_io[i]
            ld = xo.stride(0)
            lin = ln_gemm((i, "dyn"), xin, w["n1w"], w["n1b"], w["dyn_w"], w["dyn_b"], w["dyn_f"])       # [N,5d]
            ops.dynexp_step(lin, lin.stride(0), w["qexp"], w["bexp"], c["cond"], c["key"], c["va"], c["vb"], c["wfa"],
                            c["wfb"], c["qk"], st.anc, st.row_valid, st.pos, xin, ld, xo, ld, N, st.T, d,
                            g.num_exp_dec)
            q = ln_gemm((i, "wq"), xo, w["n2w"], w["n2b"], w["wq"], w["bq"], w["wq_f"])
            att = torch.empty(N, d, dtype=torch.float32, device=self.device)
            ops.cross_attn_step(q, d, st.kv, st.kv.shape[2], 2 * i * d, (2 * i + 1) * d, st.enc_len,
                                st.row_valid, att, d, N, st.n_img, st.S, d, g.num_heads)
            gemm((i, "wo"), att, w["wo"], w["bo"], xo, xo)
            h = ln_gemm((i, "f1"), xo, w["n3w"], w["n3b"], w["f1w"], w["f1b"], w["f1_f"], act=ops.ACT_RELU)
            gemm((i, "f2"), h, w["f2w"], w["f2b"], xo, xo)
        pre = torch.empty(N, d, dtype=torch.float32, device=self.device)
        gemm("reduce", st.ycat, self.dr_w, self.dr_b, st.layer_io[-1][1], pre)
        if fuse:
            gemm("vocab", pre, self.voc_f[0], self.voc_f[1], out=st.logits, ln_fold=(self.voc_f[2], eps))
        else:
            gemm("vocab", ops.layernorm(pre, self.drn_w, self.drn_b), self.voc_w, self.voc_b, out=st.logits)

    def search_constraints(self, st: DecodeState, eos_idx: int, *, no_repeat_ngram: int = 0, min_words: int = 0,
                           banned=None) -> Optional["_hip.SearchConstraints"]:
        """The constraints of a search on `st` for beam_step / group_beam_step, or None when none is
        active: words that would repeat an n-gram of the row's prefix, EOS before `min_words` words, the word ids in
        `banned`.  The arguments pass search.check_constraints (as no_repeat_ngram_size, min_length, banned_words of a
        caption of st.T positions).  Everything the kernel reads is device resident (st.tokens, st.pos, st.row_valid, the
        uploaded ban list)."""
        c = check_constraints(no_repeat_ngram, min_words, banned, V=self.g.vocab_size, max_seq_len=st.T,
                              rows_per_image=st.beams, sos_idx=None, eos_idx=eos_idx)
        if c is None:
            return None
        st.banned = torch.tensor(c["banned"], dtype=torch.int32, device=self.device) if c["banned"] else None
        return ops.search_constraints(st.tokens, st.pos, st.T, eos_idx, row_valid=st.row_valid, banned=st.banned,
                                      no_repeat_ngram=min(c["no_repeat_ngram"], st.T), min_words=c["min_words"])

    def constrained_candidates(self, st: DecodeState, constraints, logp: Optional[torch.Tensor] = None) -> None:
        """st.cand_val / st.cand_idx = the st.beams best ADMISSIBLE words of every row.  The rows are the log-probs the
        unconstrained launch writes (logp_out of odic_logsoftmax_topk into st.logp) or, given `logp`, rows that are
        log-probs already (the ensemble's average); odic_topk_rows_constrained selects from them as they are."""
        V = self.g.vocab_size
        if logp is None:
            if st.logp is None:
                st.logp = torch.empty(st.N, V, dtype=torch.float32, device=self.device)
            logp = st.logp
            ops.logsoftmax_topk(st.logits, V, logp, V, st.cand_val, st.cand_idx, st.N, V, st.beams)
        ops.topk_rows_constrained(logp, constraints, st.cand_val, st.cand_idx, st.beams)

    def _candidates(self, st: DecodeState, constraints, want_logp: bool = False) -> None:
        """The decoder pass of a step, then st.cand_val / st.cand_idx = the st.beams best (admissible) words of every row.
        `want_logp`: the top-k launch also writes the log-prob rows (st.logp), as it does under constraints anyway."""
        self.step_logits(st, embed=False)
        if constraints is not None:
            self.constrained_candidates(st, constraints)
            return
        V = self.g.vocab_size
        if want_logp and st.logp is None:
            st.logp = torch.empty(st.N, V, dtype=torch.float32, device=self.device)
        logp, ldp = (st.logp, V) if want_logp else (None, 0)
        ops.logsoftmax_topk(st.logits, V, logp, ldp, st.cand_val, st.cand_idx, st.N, V, st.beams)

    def beam_step(self, st: DecodeState, eos_idx: int, constraints=None) -> None:
        """One full search step: decoder → log-softmax / top-k (one block per row) → beam bookkeeping + the next
        position's input rows (one block per image).  The state must have been armed with
        ops.beam_reset(st.beam_state, ..., emb=st.emb).  (Both launches in one were slower, DESIGN.md §4.6: a block
        per image then works through its k rows alone.)  `constraints` (search_constraints(st, ...)): the top-k launch
        also writes the log-prob rows, and odic_topk_rows_constrained re-selects the candidates from them."""
        self._candidates(st, constraints)
        ops.beam_step(st.cand_val, st.cand_idx, st.beam_state, st.n_img, st.beams, st.T, eos_idx, emb=st.emb)

    def group_beam_step(self, st: DecodeState, eos_idx: int, groups: int, penalty: float, constraints=None) -> None:
        """One full step of diverse beam search, the sibling of beam_step: all st.beams = groups·k' rows of an image go
        through the decoder and the top-k launch together (k = st.beams candidates per row); only the selection walks
        the groups in turn (odic_group_beam_step, one block per image)."""
        if groups < 1 or st.beams % groups:
            raise ValueError(f"{st.beams} rows per image do not split into {groups} groups")
        self._candidates(st, constraints)
        ops.group_beam_step(st.cand_val, st.cand_idx, st.beam_state, st.n_img, groups, st.beams // groups, st.T, eos_idx,
                            penalty, emb=st.emb)

    def require_beam_step(self, st: DecodeState, eos_idx: int, required: torch.Tensor, bank_beams: int,
                          constraints=None) -> None:
        """One full step of a search whose captions must contain given words, the sibling of beam_step:
        `required` int64 [n_img, C] on the device (-1 = unused slot), st.beams = 2^C·bank_beams rows per image.  The top-k
        launch always writes the log-prob rows (st.logp, k = st.beams): a required word need not be among a row's
        candidates, so odic_require_beam_step reads its log-prob there.  `constraints`: as in beam_step."""
        C = int(required.shape[1])
        if bank_beams < 1 or st.beams != bank_beams << C:
            raise ValueError(f"{st.beams} rows per image are not 2^{C} banks of {bank_beams} beams")
        self._candidates(st, constraints, want_logp=True)
        ops.require_beam_step(st.cand_val, st.cand_idx, st.logp, required, st.beam_state, st.n_img, bank_beams, st.T,
                              eos_idx, emb=st.emb)

    def stochastic_beam_step(self, st: DecodeState, eos_idx: int, seed: int) -> None:
        """One full step of stochastic beam search, the sibling of beam_step with the same two launches
        behind the decoder: st.beams draws without replacement per row WITH their perturbed scores
        (odic_logsoftmax_sample_scored, noise keyed by `seed`, the row, the word and *st.pos) into st.cand_val / cand_idx /
        cand_pert, then odic_stochastic_beam_step, which keeps the st.beams best perturbed continuations of every image and
        carries their scores in st.gscore.  The state must have been armed like beam_step's."""
        if st.cand_pert is None:
            st.cand_pert = torch.empty(st.N, st.beams, dtype=torch.float32, device=self.device)
            st.gscore = torch.empty(st.N, dtype=torch.float32, device=self.device)
        V = self.g.vocab_size
        self.step_logits(st, embed=False)
        ops.logsoftmax_sample_scored(st.logits, V, None, 0, st.cand_val, st.cand_idx, st.cand_pert, st.N, V, st.beams, seed,
                                     st.pos)
        ops.stochastic_beam_step(st.cand_val, st.cand_idx, st.cand_pert, st.gscore, st.beam_state, st.n_img, st.beams,
                                 st.T, eos_idx, emb=st.emb)

    def pool_constraints(self, st: DecodeState, eos_idx: int, *, no_repeat_ngram: int = 0, banned=None
                         ) -> "_hip.SearchConstraints":
        """The constraints every pooled step selects its candidates under: the search's own n-gram rule
        and ban list, and EOS inadmissible at every position (min_words = st.T: odic_pool_beam_step offers EOS itself, from
        the log-prob rows, and applies min_length there) — so a row's candidates are its st.beams best words other than
        EOS, exactly."""
        banned = sorted({int(w) for w in (banned or [])})
        if len(banned) + st.T + st.beams > self.g.vocab_size:
            raise ValueError(f"{len(banned)} banned words + {st.T} positions + {st.beams} candidates per row exceed the "
                             f"vocabulary ({self.g.vocab_size} words): a row could run out of admissible words")
        st.banned = torch.tensor(banned, dtype=torch.int32, device=self.device) if banned else None
        return ops.search_constraints(st.tokens, st.pos, st.T, eos_idx, row_valid=st.row_valid, banned=st.banned,
                                      no_repeat_ngram=min(int(no_repeat_ngram), st.T), min_words=st.T)

    def pool_beam_step(self, st: DecodeState, pool: "ops.Pool", eos_idx: int, constraints) -> None:
        """One full step of pooled beam search, the sibling of beam_step under constraints with the same
        launches behind the decoder: the top-k launch that writes the log-prob rows, odic_topk_rows_constrained under
        `constraints` (pool_constraints: never EOS), then odic_pool_beam_step, which offers every row's EOS from the
        log-prob rows, moves the hypotheses that end to `pool` and keeps st.beams live rows."""
        self._candidates(st, constraints)
        ops.pool_beam_step(st.cand_val, st.cand_idx, st.logp, pool.args, st.beam_state, st.n_img, st.beams, st.T, eos_idx,
                           emb=st.emb)

    def contrast_beam_step(self, states, count: torch.Tensor, args: "_hip.ContrastArgs", eos_idx: int,
                           constraints=None) -> None:
        """One full step of contrastive beam search, the sibling of beam_step: states[0] decodes the
        target images, the others the distractor images (the same rows against other encoder memories), all on
        search.share_beam_state(states) and embedding for themselves like the members of an ensemble.  A decoder pass per
        state, then ONE launch that turns the 1 + D logits rows of every beam into contrastive scores and their st.beams
        best (odic_contrast_topk; count int32 [N]: the distractors row n uses), then the unchanged odic_beam_step.
        `constraints`: the launch also writes the score rows (lead.logp) and odic_topk_rows_constrained re-selects the
        candidates from them; args.min_keep then covers what a row can lose."""
        lead = states[0]
        for st in states:
            self.step_logits(st)                                     # private caches, shared next_tok / pos / ancestors
        score = None
        if constraints is not None:
            if lead.logp is None:
                lead.logp = torch.empty(lead.N, self.g.vocab_size, dtype=torch.float32, device=self.device)
            score = lead.logp
        ops.contrast_topk([st.logits for st in states], count, args, lead.cand_val, lead.cand_idx, lead.beams,
                          score_out=score)
        if constraints is not None:
            ops.topk_rows_constrained(score, constraints, lead.cand_val, lead.cand_idx, lead.beams)
        ops.beam_step(lead.cand_val, lead.cand_idx, lead.beam_state, lead.n_img, lead.beams, lead.T, eos_idx)

    # ------------------------------------------------------------------------------------------
    # a search that starts behind a given prefix
    def prefill(self, st: DecodeState, prefix: torch.Tensor, sos_idx: int, want_logits: bool = False):
        """One whole-sequence pass over [sos, w_1 .. w_{P-1}] per image (n_img rows per position) that also fills the
        step caches of `st` for positions 0..P-1, slot = the image's first row.  prefix int64 [n_img, P] on the device.
        → the model's log-probs of the prefix words fp32 [n_img, P], or with want_logits the logits [n_img, P, V]."""
        n_img, P = prefix.shape
        if n_img != st.n_img or not 1 <= P <= st.T - 2:
            raise ValueError(f"a prefix of {P} words for {n_img} images does not fit a state of {st.n_img} images and "
                             f"{st.T} positions")
        dec = torch.cat([torch.full((n_img, 1), int(sos_idx), dtype=torch.int64, device=self.device), prefix[:, :-1]], 1)
        dec_len = torch.full((n_img,), P, dtype=torch.int32, device=self.device)
        if want_logits:
            return self.decode_sequence(dec, dec_len, st.kv, st.enc_len, n_img, want_logits=True, fill=(st, st.beams))
        return self.decode_sequence(dec, dec_len, st.kv, st.enc_len, n_img, targets=prefix.contiguous(),
                                    fill=(st, st.beams))["logp"]

    def seed_prefix(self, st: DecodeState, prefix: torch.Tensor, sos_idx: int, group_beams: Optional[int] = None) -> None:
        """Arm `st` for a search that continues `prefix` (int64 [n_img, P], the same P for every image): prefill, then
        odic_beam_reset_prefix — every row holds [sos, prefix] with the prefix words' own log-probs, *pos = P, and only
        the first row of every group of `group_beams` rows (default: all st.beams rows are one group) has a finite
        cumulative score, so the next beam_step / group_beam_step seeds at position P as it seeds at position 0."""
        prefix = prefix.to(self.device, torch.int64).contiguous()
        logp = self.prefill(st, prefix, sos_idx)
        ops.beam_reset_prefix(st.beam_state, prefix, logp.contiguous(), st.n_img, st.beams, group_beams or st.beams, st.T,
                              sos_idx, emb=st.emb)

    # ------------------------------------------------------------------------------------------
    # whole-sequence (teacher-forced) pass: every token is known, so the N·T rows go through each layer at once
    def vocab_row_chunk(self) -> int:
        """Rows per vocabulary product of decode_sequence: the logits workspace stays below 100 MB (2496 rows at
        V = 10000)."""
        return max(64, (100_000_000 // (4 * self.g.vocab_size)) // 64 * 64)

    def decode_sequence(self, tokens: torch.Tensor, dec_len: torch.Tensor, kv: torch.Tensor, enc_len: torch.Tensor,
                        n_img: int, targets: Optional[torch.Tensor] = None, want_logits: bool = False,
                        row_chunk: Optional[int] = None, attn: Optional[dict] = None, fill: Optional[tuple] = None):
        """Teacher-forced decoder over whole sequences (End_ExpansionNet_v2.py:103-138 in one pass).
        tokens int64 [N, T], rows image-major (N / n_img captions per image, sharing that image's K/V); dec_len int32 [N]
        real tokens per row; kv = project_kv(mem) [n_img, S, 2·N_dec·d]; enc_len int32 [n_img].
        want_logits: returns the logits fp32 [N, T, V] (padded rows hold what the reference's masked rows hold).
        Otherwise returns a dict of per-position statistics, each [N, T]: 'logp' (log-prob of targets[n, t]; only with
        `targets` int64 [N, T]), 'sum_logp' (Σ_v log-prob), 'argmax' (int32), 'max_logp', and 'status' (int32 scalar,
        non-zero when a target was outside the vocabulary).  The vocabulary product and the statistics run over
        `row_chunk` rows at a time; the chunking changes no result bit (every product here is the 64 x 64 tile kernel,
        whose rows are independent of M).  The number of launches does not depend on T.
        attn = {"layers": [i, …], "per_head": bool, "reduce_layers": bool}: the statistics gain 'attn', the cross-attention
        probabilities of the listed decoder layers (odic_cross_attn_probs on the q, kv, enc_len and row mask the layer's
        attention runs on; one more launch per listed layer): fp32 [N, T, S] with reduce_layers (the mean over the listed
        layers), [N, L', T, S] without, the mean over the heads either way; with per_head a heads axis in front of T.
        Padded rows hold the uniform 1/S of a masked row.  Without `attn` nothing is allocated or launched for it, and
        every other result keeps its bits either way.
        fill = (state, rows_per_image): every layer also writes the step caches of `state` (a DecodeState) for positions
        0..T-1 of sequence i into slot i·rows_per_image, from the layer's `lin` rows (odic_dynexp_fill_caches; one more
        launch per layer) — a search on `state` can then go on from position T (seed_prefix).  Without `fill` nothing is
        allocated or launched for it, and every result keeps its bits either way."""
        g, dv = self.g, self.device
        d, L, V, E = g.d_model, g.N_dec, g.vocab_size, g.num_exp_dec
        N, T = tokens.shape
        if T > 128:
            raise RuntimeError("more than 128 decode positions are not supported by odic_dynexp_seq")
        if T > self.pos_table.shape[0]:
            raise RuntimeError(f"{T} decode positions exceed the pos_encoder table ({self.pos_table.shape[0]})")
        if N % n_img or kv.shape[0] != n_img or enc_len.numel() != n_img or dec_len.numel() != N:
            raise RuntimeError("decode_sequence: rows must be image-major with N a multiple of n_img")
        if tokens.dtype != torch.int64 or dec_len.dtype != torch.int32 or enc_len.dtype != torch.int32:
            raise RuntimeError("decode_sequence wants int64 tokens and int32 lengths")
        tokens = tokens.contiguous()
        M, S = N * T, kv.shape[1]
        f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dv)      # noqa: E731
        TC = 3                                   # odic_gemm tile_cfg: the 64 x 64 tile kernel whatever M is
        ycat, row_valid = f(M, L * d), torch.empty(M, dtype=torch.int32, device=dv)
        ld = ycat.stride(0)
        ops.dec_embed_seq(tokens, self.embed, self.pos_table, ycat, ld, N, T, d, math.sqrt(d), dec_len, row_valid)
        xn, lin, q, att, h = f(M, d), f(M, 5 * d), f(M, d), f(M, d), f(M, g.ff)
        amap = None
        if attn is not None:
            if want_logits:
                raise RuntimeError("decode_sequence: attn comes with the statistics, not with want_logits")
            a_layers = [int(i) for i in attn["layers"]]
            if not a_layers or len(set(a_layers)) != len(a_layers) or min(a_layers) < 0 or max(a_layers) >= L:
                raise ValueError(f"attn layers must be distinct indices in [0, {L})")
            a_heads, a_reduce = bool(attn.get("per_head", False)), bool(attn.get("reduce_layers", False))
            H = g.num_heads
            a_w = H * S if a_heads else S
            amap = f(1 if a_reduce else len(a_layers), M, a_w)
            a_scale = (1.0 if a_heads else 1.0 / H) / (len(a_layers) if a_reduce else 1)
        for i, w in enumerate(self.dec):
            xo = ycat[:, i * d:(i + 1) * d]
            xin = xo if i == 0 else ycat[:, (i - 1) * d:i * d]             # (layer 0 works in place)
            ops.layernorm(xin, w["n1w"], w["n1b"], out=xn)
            ops.gemm(xn, w["dyn_w"], w["dyn_b"], out=lin, tile_cfg=TC)                                   # [M,5d]
            ops.dynexp_seq(lin, lin.stride(0), w["qexp"], w["bexp"], dec_len, xin, ld, xo, ld, N, T, d, E)
            if fill is not None:
                ops.dynexp_fill_caches(lin, lin.stride(0), w["qexp"], fill[0].caches[i], N, T, int(fill[1]), fill[0].N, fill[0].T,
                                       d, E)
            ops.layernorm(xo, w["n2w"], w["n2b"], out=xn)
            ops.gemm(xn, w["wq"], w["bq"], out=q, tile_cfg=TC)
            # the step kernel's row → image map is row / (rows / n_img): the sequence-major rows of an image are contiguous
            ops.cross_attn_step(q, d, kv, kv.shape[2], 2 * i * d, (2 * i + 1) * d, enc_len, row_valid, att, d, M,
                                n_img, S, d, g.num_heads)
            if amap is not None and i in a_layers:
                j = a_layers.index(i)
                ops.cross_attn_probs(q, d, kv, kv.shape[2], 2 * i * d, enc_len, row_valid, amap[0 if a_reduce else j], a_w,
                                     M, n_img, S, d, g.num_heads, per_head=a_heads, accumulate=a_reduce and i != min(a_layers),
                                     scale=a_scale)
            ops.gemm(att, w["wo"], w["bo"], residual=xo, out=xo, tile_cfg=TC)
            ops.layernorm(xo, w["n3w"], w["n3b"], out=xn)
            ops.gemm(xn, w["f1w"], w["f1b"], out=h, act=ops.ACT_RELU, tile_cfg=TC)
            ops.gemm(h, w["f2w"], w["f2b"], residual=xo, out=xo, tile_cfg=TC)
        pre = f(M, d)
        ops.gemm(ycat, self.dr_w, self.dr_b, residual=ycat[:, (L - 1) * d:], out=pre, tile_cfg=TC)
        ops.layernorm(pre, self.drn_w, self.drn_b, out=xn)
        rc = int(row_chunk) if row_chunk is not None else self.vocab_row_chunk()      # (0 is an error, not "the default")
        if rc <= 0:
            raise ValueError("row_chunk must be positive")
        if want_logits:
            out = f(N, T, V)
            o2 = out.view(M, V)
            for r0 in range(0, M, rc):
                r1 = min(M, r0 + rc)
                ops.gemm(xn[r0:r1], self.voc_w, self.voc_b, out=o2[r0:r1], tile_cfg=TC)
            return out
        tg = None
        if targets is not None:
            if targets.dtype != torch.int64 or tuple(targets.shape) != (N, T):
                raise RuntimeError("targets must be int64 [N, T]")
            tg = targets.contiguous().view(M)
        logp = f(M) if tg is not None else None
        sum_logp, max_logp = f(M), f(M)
        argmax = torch.empty(M, dtype=torch.int32, device=dv)
        status = torch.zeros(1, dtype=torch.int32, device=dv)
        ws = f(min(rc, M), V)
        for r0 in range(0, M, rc):
            r1 = min(M, r0 + rc)
            ops.gemm(xn[r0:r1], self.voc_w, self.voc_b, out=ws[:r1 - r0], tile_cfg=TC)
            ops.token_stats(ws, V, None if tg is None else tg[r0:r1], None if logp is None else logp[r0:r1],
                            sum_logp[r0:r1], argmax[r0:r1], max_logp[r0:r1], None if tg is None else status, r1 - r0, V)
        res = {"sum_logp": sum_logp.view(N, T), "argmax": argmax.view(N, T), "max_logp": max_logp.view(N, T),
               "status": status}
        if logp is not None:
            res["logp"] = logp.view(N, T)
        if amap is not None:
            a = amap.view(amap.shape[0], N, T, H, S).permute(1, 0, 3, 2, 4) if a_heads else \
                amap.view(amap.shape[0], N, T, S).transpose(0, 1)                  # [N, L', (H,) T, S]
            res["attn"] = (a[:, 0] if a_reduce else a).contiguous()
        return res
