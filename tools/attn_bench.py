#!/usr/bin/env python3
"""Isolated timing of odic_window_attention per Swin-L stage at batch B: table kernel vs packed-bias kernel (bf16), or the
packed-bias kernel alone for fp16 / split-fp16 activations.  Prints µs per launch and algorithmic TB/s (36,864 B per
(window, head) at 16 bits).   python tools/attn_bench.py [16] [--dtype bf16|fp16|h2] [--lib other/libodic_hip.so]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from on_device_image_captioning_amd import _hip

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=16)
ap.add_argument("--dtype", choices=("bf16", "fp16", "h2"), default="bf16")
ap.add_argument("--lib", help="time this build of the library instead of the tree's")
a = ap.parse_args()
if a.lib:
    _hip.LIB_PATH = os.path.abspath(a.lib)
from on_device_image_captioning_amd import ops

B = a.B
torch.manual_seed(0)
for res, heads in ((96, 6), (48, 12), (24, 24), (12, 48)):
    C = heads * 32
    qkv = torch.randn(B * res * res, 3 * C, device="cuda")
    qkv = ops.h2_from_f32(qkv) if a.dtype == "h2" else qkv.to(torch.bfloat16 if a.dtype == "bf16" else torch.float16)
    table = (torch.randn(529, heads, device="cuda") * 0.1)
    dense = ops.shifted_bias_prescaled(table, 12, 32 ** -0.5)
    out = torch.empty(B * res * res, C, device="cuda", dtype=qkv.dtype)
    inst = B * (res // 12) ** 2 * heads
    for shift in (0, 6 if res > 12 else 0):
        cells = []
        for name, kw in (("table", {}), ("packed", {"bias_shifted_prescaled": dense}))[a.dtype != "bf16":]:
            for _ in range(3):
                ops.window_attention(qkv, table, B, res, C, heads, 12, shift, out=out, **kw)
            torch.cuda.synchronize()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            for _ in range(20):
                ops.window_attention(qkv, table, B, res, C, heads, 12, shift, out=out, **kw)
            en.record(); torch.cuda.synchronize()
            us = st.elapsed_time(en) * 1e3 / 20
            cells.append(f"{name} {us:7.1f} us {inst * 18432 * qkv.element_size() / us / 1e6:6.2f} TB/s")
        print(f"res {res:3d} heads {heads:2d} shift {shift}  instances {inst:6d} | " + " | ".join(cells))
