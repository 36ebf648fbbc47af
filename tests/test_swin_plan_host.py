"""Which launches a Swin block takes (engine.swin_block_plan), for every precision and every ODIC_FUSE_* setting, on the CPU.

The table below was written out by hand from the block loop of SwinEngine.forward as it stood before the chooser existed
(one three-way `if` on fp8 / folded weights / plain, with the fusions nested inside), not produced by the chooser.  Per
(precision, environment): "attention/MLP" for the four Swin-L stages and for one odd block — width 192 at resolution 12,
one image, M = 144 rows, which is no multiple of 128, so the LayerNorm-while-reading and the fused-MLP kernels refuse it.
At the four stages M is 9216 / 2304 / 576 / 144 per image; one image and sixteen take the same forms.

What a block carries follows from how SwinEngine packs it: the packed attention bias in every mode but fp32 (12 x 12
windows everywhere here), the folded `*_lnr` weights at width 192 when `ln_read` is on, a qkv operand without a pack-time
scale in every mode but x3.
"""
import pytest

from on_device_image_captioning_amd.engine import SwinFlags, swin_block_plan

FLAGS = ("ODIC_FUSE_BACKBONE_LN_READ", "ODIC_FUSE_QKV_ATTENTION", "ODIC_FUSE_QKV_ATTENTION_TILED",
         "ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C", "ODIC_FUSE_MLP", "ODIC_SWIN_CHUNKS")
SETTINGS = {"default": {}, "ln_read=0": {"ODIC_FUSE_BACKBONE_LN_READ": "0"}, "qkv_attention=0": {"ODIC_FUSE_QKV_ATTENTION": "0"},
            "tiled=0": {"ODIC_FUSE_QKV_ATTENTION_TILED": "0"}, "mlp=0": {"ODIC_FUSE_MLP": "0"},
            "ln_read=x3": {"ODIC_FUSE_BACKBONE_LN_READ": "x3"}, "min_c=384": {"ODIC_FUSE_QKV_ATTENTION_TILED_MIN_C": "384"}}
#: (C, heads, res, rows per image) — Swin-L's stages, then the odd block
BLOCKS = [(192, 6, 96, 96 * 96), (384, 12, 48, 48 * 48), (768, 24, 24, 24 * 24), (1536, 48, 12, 12 * 12), (192, 6, 12, 144)]
WS = 12

ALL_PLAIN = "plain/plain plain/plain plain/plain plain/plain plain/plain"
ALL_FP8 = "fp8/fp8 fp8/fp8 fp8/fp8 fp8/fp8 fp8/fp8"
BF16_DEFAULT = "fused/fused plain/plain tiled/plain tiled/plain plain/plain"
#: precision ("fp8+" = fp8 with its calibration done, "fp8-" = before) → setting → forms outside a calibration pass
PLANS = {
    "fp32": {k: ALL_PLAIN for k in SETTINGS},
    "x3": {"default": ALL_PLAIN, "ln_read=0": ALL_PLAIN, "qkv_attention=0": ALL_PLAIN, "tiled=0": ALL_PLAIN, "mlp=0": ALL_PLAIN,
           "ln_read=x3": "ln_read/ln_read plain/plain plain/plain plain/plain plain/plain", "min_c=384": ALL_PLAIN},
    "fp8+": {k: ALL_FP8 for k in SETTINGS},
    "fp8-": {k: ALL_PLAIN for k in SETTINGS},
    "bf16": {"default": BF16_DEFAULT,
             "ln_read=0": "plain/plain plain/plain tiled/plain tiled/plain plain/plain",
             "qkv_attention=0": "ln_read/fused plain/plain tiled/plain tiled/plain plain/plain",
             "tiled=0": "fused/fused plain/plain plain/plain plain/plain plain/plain",
             "mlp=0": "fused/ln_read plain/plain tiled/plain tiled/plain plain/plain",
             "ln_read=x3": BF16_DEFAULT,
             "min_c=384": "fused/fused tiled/plain tiled/plain tiled/plain plain/plain"},
}


def plans(monkeypatch, mode, setting, calibrating):
    """The chooser's answers for the five blocks, at one image and at sixteen (the odd block: one image only)."""
    for k in FLAGS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    precision = mode.rstrip("+-")
    flags = SwinFlags.from_env(precision)
    got = {}
    for n_img in (1, 16):
        row = []
        for i, (C_, heads, res, rows) in enumerate(BLOCKS):
            M = rows * (n_img if i < 4 else 1)
            attn, mlp = swin_block_plan(precision, flags, C_, heads, WS, res, M, dense=precision != "fp32",
                                        folded=flags.ln_read and C_ == 192, qkv_a_one=precision != "x3",
                                        calibrating=calibrating, fp8_ready=mode == "fp8+")
            row.append(f"{attn}/{mlp}")
        got[n_img] = " ".join(row)
    return got


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mode", list(PLANS))
def test_the_chooser_gives_the_forms_the_block_loop_took(monkeypatch, mode, setting):
    got = plans(monkeypatch, mode, setting, calibrating=False)
    assert got[1] == PLANS[mode][setting], (mode, setting)
    assert got[16] == PLANS[mode][setting], (mode, setting)


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("mode", list(PLANS))
def test_a_calibration_pass_takes_the_plain_forms(monkeypatch, mode, setting):
    """`_amax` taps need the LayerNorm outputs and the hidden activations in memory: only the plain forms write them."""
    assert plans(monkeypatch, mode, setting, calibrating=True) == {1: ALL_PLAIN, 16: ALL_PLAIN}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_a_calibrated_fp8_engine_takes_the_fp8_forms(monkeypatch, setting):
    assert plans(monkeypatch, "fp8+", setting, calibrating=False) == {1: ALL_FP8, 16: ALL_FP8}


def test_the_flags_keep_their_defaults_and_their_precision_gates(monkeypatch):
    for k in FLAGS:
        monkeypatch.delenv(k, raising=False)
    on = SwinFlags(ln_read=True, fuse_qkv_attn=True, fuse_qkv_attn_tiled=True, fuse_qkv_attn_tiled_min_c=768, fuse_mlp=True,
                   stage_chunks=[1])
    off = SwinFlags(ln_read=False, fuse_qkv_attn=False, fuse_qkv_attn_tiled=False, fuse_qkv_attn_tiled_min_c=768,
                    fuse_mlp=False, stage_chunks=[1])
    assert SwinFlags.from_env("bf16") == on
    assert all(SwinFlags.from_env(p) == off for p in ("fp32", "x3", "fp8"))
    monkeypatch.setenv("ODIC_FUSE_BACKBONE_LN_READ", "x3")                   # split fp16 opts in with =x3, bf16 stays on
    monkeypatch.setenv("ODIC_SWIN_CHUNKS", "4,2")
    assert SwinFlags.from_env("x3").ln_read and SwinFlags.from_env("bf16").ln_read and not SwinFlags.from_env("fp32").ln_read
    assert SwinFlags.from_env("bf16").stage_chunks == [4, 2]
    monkeypatch.setenv("ODIC_FUSE_BACKBONE_LN_READ", "1")
    assert not SwinFlags.from_env("x3").ln_read
