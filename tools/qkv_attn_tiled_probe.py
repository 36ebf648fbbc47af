#!/usr/bin/env python3
"""qkv -> attention core of a Swin block at batch B, stages 1-3 of Swin-L: the tiled product (tile_cfg 41, and the tuner's
A-resident choice where it applies) + window attention (two launches) against odic_swin_qkv_attention_tiled (one), isolated,
interleaved.
python tools/qkv_attn_tiled_probe.py [16]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from on_device_image_captioning_amd import ops

B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ws = 12
torch.manual_seed(0)
for name, res, C, heads, shift in (("stage2", 24, 768, 24, 6), ("stage2", 24, 768, 24, 0), ("stage3", 12, 1536, 48, 0),
                                   ("stage1", 48, 384, 12, 6)):
    M = B * res * res
    xn = torch.randn(M, C, device="cuda").bfloat16()
    W = (torch.randn(3 * C, C, device="cuda") * C ** -0.5).bfloat16()
    b = torch.randn(3 * C, device="cuda")
    table = torch.randn(529, heads, device="cuda") * 0.1
    dense = ops.shifted_bias_prescaled(table, ws, 32 ** -0.5)
    qkv = torch.empty(M, 3 * C, device="cuda", dtype=torch.bfloat16)
    out = torch.empty(M, C, device="cuda", dtype=torch.bfloat16)
    fns = {"qkv(cfg41)": lambda: ops.gemm(xn, W, b, out=qkv, tile_cfg=41),
           "attention": lambda: ops.window_attention(qkv, table, B, res, C, heads, ws, shift, out=out, bias_shifted_prescaled=dense),
           "fused": lambda: ops.swin_qkv_attention_tiled(xn, W, b, dense, B, res, C, heads, ws, shift, out=out)}
    if C == 384:
        fns["qkv(cfg53)"] = lambda: ops.gemm(xn, W, b, out=qkv, tile_cfg=53)
    t = {k: [] for k in fns}
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    for _ in range(7):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                f()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) * 100)
    print(f"{name} B={B} res{res} C{C} shift {shift}: " + "  ".join(f"{k} {sorted(v)[3]:.1f} us" for k, v in t.items()), flush=True)
