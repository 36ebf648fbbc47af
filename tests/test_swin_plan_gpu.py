"""What one SwinEngine.forward enqueues, per precision and per ODIC_FUSE_* setting (`-m gpu`): Swin-L with two blocks per
stage — a width-192 stage whose row count is a multiple of 128, two stages the tiled qkv → core launch takes (768 and 1536:
heads x 32 = width, heads in threes, 12 x 12 windows), a shifted and an unshifted block wherever the resolution allows —
synthetic backbone weights, one image; two images with ODIC_SWIN_CHUNKS=2,2 for the chunked block loop.

The launch families (the names ops.py gives its launches: both fused qkv → core kernels count as "swin_qkv_attention", the
fp16 attention core of the fp8 mode as "window_attention_bf16") are compared with the lists written out below; they are what
tools/swin_trace.py printed before the block loop was rewritten around engine.swin_block_plan
(profiles/r18_swin_trace_parent.txt).

Bits: the one-launch forms are documented bit-identical to the launches they replace.  Through the
engine, on this geometry, all three equalities held before the rewrite — ODIC_FUSE_QKV_ATTENTION=0, ODIC_FUSE_MLP=0 and
ODIC_FUSE_QKV_ATTENTION_TILED=0 each give the default's features bit for bit — so all three are asserted.
ODIC_FUSE_BACKBONE_LN_READ=0 is documented as NOT bit-identical (gamma folded into rounded weights) and is not compared.
"""
import dataclasses

import pytest
import torch

from on_device_image_captioning_amd import ops
from on_device_image_captioning_amd import weights as W

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda:0"
G = dataclasses.replace(W.FULL, swin_depths=(2, 2, 2, 2))
FLAGS = ("ODIC_FUSE_BACKBONE_LN_READ", "ODIC_FUSE_QKV_ATTENTION", "ODIC_FUSE_QKV_ATTENTION_TILED",
         "ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C", "ODIC_FUSE_MLP", "ODIC_SWIN_CHUNKS")


def plain(gemm, core):
    return ["layernorm", gemm, core, gemm, "layernorm", gemm, gemm]


# one block, by the forms of its two halves (proj + residual between them)
F32, X3 = plain("gemm_f32", "window_attention_f32"), plain("gemm_x3", "window_attention_x3")
BF16 = plain("gemm_bf16", "window_attention_bf16")
X3_LN_READ = ["gemm_x3", "window_attention_x3", "gemm_x3", "gemm_x3", "gemm_x3"]
FP8 = ["layernorm", "gemm_fp8", "window_attention_bf16", "gemm_f16", "layernorm", "gemm_fp8", "gemm_fp8"]
FUSED_FUSED = ["swin_qkv_attention", "gemm_bf16", "swin_mlp"]
LN_READ_FUSED = ["gemm_bf16", "window_attention_bf16", "gemm_bf16", "swin_mlp"]
FUSED_LN_READ = ["swin_qkv_attention", "gemm_bf16", "gemm_bf16", "gemm_bf16"]
TILED = ["layernorm", "swin_qkv_attention", "gemm_bf16", "layernorm", "gemm_bf16", "gemm_bf16"]


def backbone(stages, merge_gemm, chunks=(1, 1, 1, 1)):
    """patch embedding, per stage its two blocks (once per image chunk) and the patch merge behind it, the final norm."""
    fam = ["patch_embed"]
    for s, block in enumerate(stages):
        fam += (block + block) * chunks[s] + (["patch_merge_layernorm", merge_gemm] if s < 3 else [])
    return fam + ["layernorm"]


BF16_DEFAULT = [FUSED_FUSED, BF16, TILED, TILED]
#: name → (precision, environment, images, families)
CONFIGS = {
    "fp32": ("fp32", {}, 1, backbone([F32] * 4, "gemm_f32")),
    "x3": ("x3", {}, 1, backbone([X3] * 4, "gemm_x3")),
    "x3 ln_read=x3": ("x3", {"ODIC_FUSE_BACKBONE_LN_READ": "x3"}, 1, backbone([X3_LN_READ, X3, X3, X3], "gemm_x3")),
    "fp8": ("fp8", {}, 1, backbone([FP8] * 4, "gemm_bf16")),
    "bf16": ("bf16", {}, 1, backbone(BF16_DEFAULT, "gemm_bf16")),
    "bf16 ln_read=0": ("bf16", {"ODIC_FUSE_BACKBONE_LN_READ": "0"}, 1, backbone([BF16, BF16, TILED, TILED], "gemm_bf16")),
    "bf16 qkv_attention=0": ("bf16", {"ODIC_FUSE_QKV_ATTENTION": "0"}, 1, backbone([LN_READ_FUSED, BF16, TILED, TILED], "gemm_bf16")),
    "bf16 tiled=0": ("bf16", {"ODIC_FUSE_QKV_ATTENTION_TILED": "0"}, 1, backbone([FUSED_FUSED, BF16, BF16, BF16], "gemm_bf16")),
    "bf16 mlp=0": ("bf16", {"ODIC_FUSE_MLP": "0"}, 1, backbone([FUSED_LN_READ, BF16, TILED, TILED], "gemm_bf16")),
    "bf16 min_c=384": ("bf16", {"ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C": "384"}, 1,
                       backbone([FUSED_FUSED, TILED, TILED, TILED], "gemm_bf16")),
    "bf16 chunks=2,2": ("bf16", {"ODIC_SWIN_CHUNKS": "2,2"}, 2, backbone(BF16_DEFAULT, "gemm_bf16", chunks=(2, 2, 1, 1))),
    "bf16, two images": ("bf16", {}, 2, backbone(BF16_DEFAULT, "gemm_bf16")),
}


@pytest.fixture(scope="module")
def state_dict():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return {name: W.synth_tensor(name, shape, kind, G, 0) for name, shape, kind in W.state_dict_spec(G)
            if name.startswith("swin_transf.")}


_RUNS = {}


def run(name, state_dict, monkeypatch):
    """(launch families, features) of one profiled forward of a fresh engine built under the configuration's environment."""
    if name not in _RUNS:
        from on_device_image_captioning_amd.engine import SwinEngine
        precision, env, n_img, _ = CONFIGS[name]
        for k in FLAGS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        eng = SwinEngine(state_dict, G, torch.device(DEV), precision)
        img = W.synth_images(n_img, G, seed=93).to(DEV)
        eng.forward(img)                                            # code load, the LayerNorm-while-reading tile choice
        with ops.profile() as recs:
            out = eng.forward(img).clone()
        torch.cuda.synchronize()
        _RUNS[name] = ([r[0] for r in recs], out)
    return _RUNS[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_a_forward_enqueues_the_launches_of_its_configuration(state_dict, monkeypatch, name):
    fam, out = run(name, state_dict, monkeypatch)
    print(f"{name}: {len(fam)} launches")
    assert fam == CONFIGS[name][3]
    assert out.shape == (CONFIGS[name][2], 144, 1536) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("name", ["bf16 qkv_attention=0", "bf16 mlp=0", "bf16 tiled=0"])
def test_a_fallback_form_gives_the_default_features_bit_for_bit(state_dict, monkeypatch, name):
    want, got = run("bf16", state_dict, monkeypatch)[1], run(name, state_dict, monkeypatch)[1]
    assert torch.equal(got, want), (name, float((got - want).abs().max()))


def test_image_chunks_give_the_whole_batch_features_bit_for_bit(state_dict, monkeypatch):
    want, got = run("bf16, two images", state_dict, monkeypatch)[1], run("bf16 chunks=2,2", state_dict, monkeypatch)[1]
    assert torch.equal(got, want), float((got - want).abs().max())
